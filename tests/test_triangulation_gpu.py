"""Landmark triangulation with the poses held fixed on the device (ba_hip_triangulate_landmarks, k_triang.hip): against
the host restatement of the same rules, against the kernels that existed before it (residual evaluation and
linearisation at the coordinates it wrote), at the edges of the wavefront ranges, and in its effects on the engine."""
import functools

import numpy as np
import pytest

import track_cases
import triangulation_cases as tc
from ba_amd import scene
from helpers import hostcheck_lib

pytestmark = pytest.mark.gpu
EPS = tc.EPS
DEFAULT_STEP_TOL = tc.DEFAULTS["step_tolerance"]
ROUNDING = ("an accept / reject or stop decision within rounding of its threshold moves the count by one: look at the "
            "gain ratio and c of the landmark before anything else")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def noisy_case(P, L, k, seed, outliers, lm_dim):
    return tc.case_from_scene(scene.make_scene(P, L, k, lm_dim=lm_dim, seed=seed, outlier_frac=outliers), lm_dim)


@functools.lru_cache(maxsize=None)
def references(P, L, k, seed, outliers, lm_dim):
    """(host restatement, numpy restatement) at the defaults, computed once and left unchanged"""
    c = noisy_case(P, L, k, seed, outliers, lm_dim)
    return tc.triangulate_host(hostcheck_lib(), c), tc.triangulate_numpy(c)


def assert_matches_host(c, res, xw, host, numpy_final, what):
    """statuses, observation and iteration counts equal the host restatement's; accepted coordinates within
    2 step_tolerance |x| + 8 cond2(V + lambda D) eps |x| (V, lambda, D of the numpy restatement's end point), the others
    bit for bit as they were.  Returns the worst ratio to the bound."""
    hres, hxw, _ = host
    assert np.array_equal(res[:, 0], hres[:, 0]), (what, np.nonzero(res[:, 0] != hres[:, 0])[0])
    assert np.array_equal(res[:, 1], hres[:, 1]), what
    differ = np.nonzero(res[:, 2] != hres[:, 2])[0]
    assert len(differ) == 0, "%s: iteration counts differ on landmarks %s (device %s, host %s); %s" % (
        what, differ, res[differ, 2], hres[differ, 2], ROUNDING)
    worst = 0.0
    for l in range(len(res)):
        if res[l, 0] == tc.OK and l in numpy_final:
            bound = tc.coordinate_bound(c, numpy_final, l, DEFAULT_STEP_TOL)
            err = np.linalg.norm(tc.params(c, xw)[l] - tc.params(c, hxw)[l])
            worst = max(worst, err / bound)
            assert err <= bound, (what, l, err, bound)
        elif res[l, 0] not in (tc.OK, tc.NOT_CONVERGED):
            assert np.array_equal(bits(xw[l]), bits(c.x_w[l])), (what, l)
    return worst


# ---- 1. device against the host restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("lm_dim", (1, 3))
@pytest.mark.parametrize("P,L,k,seed,outliers", [(16, 60, 4, 2, 0.02), (66, 120, 3, 1, 0.0)])
def test_device_matches_host_restatement(P, L, k, seed, outliers, lm_dim):
    """numpy converges every landmark of these scenes in at most 16 iterations at the defaults: zero rows that are not OK"""
    c = noisy_case(P, L, k, seed, outliers, lm_dim)
    host, (nres, _, nfin) = references(P, L, k, seed, outliers, lm_dim)
    assert np.all(nres[:, 0] == tc.OK) and nres[:, 2].max() <= 16
    eng = tc.engine(c)
    res, xw = eng.triangulate_landmarks()
    assert np.all(res[:, 0] == tc.OK), np.nonzero(res[:, 0] != tc.OK)[0]
    worst = assert_matches_host(c, res, xw, host, nfin, "P %d LmSize %d" % (P, lm_dim))
    st = eng.triangulation_stats()
    assert st["count"]["OK"] == L and st["landmarks"] == L and st["written"] == L and st["waves_early"] == 0
    assert np.array_equal(bits(eng.get_landmarks(L)), bits(xw))
    print("device against host, P %d LmSize %d: worst |dx| / bound %.3g, %d waves, %.3f ms" % (P, lm_dim, worst, st["waves"], st["device_ms"]))
    eng.close()


# ---- 2 and 4. independent of the restatement: the kernels that exist without the feature -----------------------------
def check_against_linearisation(eng, c, res, check_error=True, gradient_tolerance=tc.DEFAULTS["gradient_tolerance"]):
    """after a writing call on a fresh engine with the robust norm off: begin_solve, eval_residuals, linearize.
    check_error (every row was written): the projection error is the sum of the final costs to (O + 16) 2^-53
    relative: all terms are positive, so this holds in any summation order.  For every OK row |rhs_l,i| / sqrt(V_ii E_l) <= gradient_tolerance + 4 k eps with V_ii and E_l
    from the Jacobians of the linearisation.  Returns the two worst ratios to those bounds."""
    O, L = len(c.pose), len(c.x_w)
    eng.begin_solve()
    ev = eng.eval_residuals()
    eng.set_pose_masks(np.zeros(len(c.poses), dtype=np.uint16))
    lin = eng.linearize()
    total = float(np.sum(res[:, 4]))
    tol = (O + 16) * 2.0 ** -53
    figures = [abs(e.proj_error - total) / total / tol for e in (ev, lin)] if check_error else [0.0, 0.0]
    print("proj_error against the sum of the costs: |difference| / (total tol) = %.3g (eval_residuals), %.3g (linearize)"
          % tuple(figures))
    _, _, jl, r = eng.get_proj_jacobians(O)
    worst_c = 0.0
    for l in np.nonzero(res[:, 0] == tc.OK)[0]:
        a = np.nonzero(c.lm == l)[0]
        J, rr = jl[a].reshape(-1, c.lm_dim), r[a].reshape(-1)
        E = rr @ rr
        if E == 0.0:
            continue
        cg = np.max(np.abs(J.T @ rr) / np.sqrt(np.sum(J * J, axis=0) * E))
        lim = gradient_tolerance + 4 * len(a) * EPS
        worst_c = max(worst_c, cg / lim)
        assert cg <= lim, (l, cg, lim, res[l])
    for f in figures:
        assert f <= 1.0, figures
    return max(figures), worst_c


@pytest.mark.parametrize("lm_dim", (1, 3))
def test_result_satisfies_existing_kernels(lm_dim):
    c = noisy_case(66, 120, 3, 1, 0.0, lm_dim)
    eng = tc.engine(c)
    res, _ = eng.triangulate_landmarks()
    worst_e, worst_c = check_against_linearisation(eng, c, res)
    print("LmSize %d: worst error ratio %.3g, worst gradient ratio %.3g" % (lm_dim, worst_e, worst_c))
    eng.close()


@pytest.mark.parametrize("lm_dim", (1, 3))
def test_failures_leave_no_trace(lm_dim):
    """2 % outliers: numpy leaves 6 (LmSize 3) and 5 (LmSize 1) landmarks without OK, four to six of them behind a camera"""
    c = noisy_case(66, 120, 3, 1, 0.02, lm_dim)
    L = len(c.x_w)
    host, (nres, _, nfin) = references(66, 120, 3, 1, 0.02, lm_dim)
    assert int(np.sum(nres[:, 0] != tc.OK)) == (6 if lm_dim == 3 else 5)
    assert 4 <= int(np.sum(nres[:, 0] == tc.BEHIND_CAMERA)) <= 6
    eng = tc.engine(c)
    res, xw = eng.triangulate_landmarks()
    bad = res[:, 0] != tc.OK
    assert 0 < bad.sum() <= 0.1 * L
    after = eng.get_landmarks(L)
    kept = ~np.isin(res[:, 0], (tc.OK, tc.NOT_CONVERGED))
    assert kept.sum() >= 4
    assert np.array_equal(bits(after[kept]), bits(c.x_w[kept])) and np.array_equal(bits(xw[kept]), bits(c.x_w[kept]))
    assert np.array_equal(bits(after), bits(xw))
    assert_matches_host(c, res, xw, host, nfin, "failures, LmSize %d" % lm_dim)
    check_against_linearisation(eng, c, res, check_error=False)     # (rows that were not written sit at their old cost)
    eng.close()


# ---- 3. kernel edges ------------------------------------------------------------------------------------------------------
EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 128, 129, 700, 32, 32, 60, 4, 0] + [6] * 40 + [64] + [5] * 30 + [0]


def edge_case(lm_dim, fov):
    """track lengths on the edges of the wavefront ranges (0, 1, 2, 63, 64, 65, 128, 129, 700; 32 + 32 and 60 + 4 fill a
    range exactly), a two-camera rig (odd residuals through camera 1, mounted a little off), inactive landmarks, and
    either per-pose intrinsics (pinhole rig) or a FOV camera 1: ba_hip_begin_solve offers per-pose intrinsics on
    pinhole rigs only, so the two cannot share an engine"""
    sc, z, pose, lm = track_cases.build(lm_dim, EDGE_LENGTHS)
    c = tc.case_from_scene(sc, lm_dim, obs=(z, pose, lm))
    c.cam_params = np.vstack([c.cam_params, c.cam_params * [1.02, 0.98, 1.0, 1.0]])
    c.cam_tvs = np.array([[0.0, 0, 0, 0, 0, 0, 1], [0.02, -0.01, 0.01, 0, 0, 0, 1]])
    c.cam_model, c.cam_w = np.zeros(2, dtype=np.int32), np.zeros(2)
    c.cam = (np.arange(len(c.pose)) % 2).astype(np.uint32)
    c.weight = 0.5 + (np.arange(len(c.pose)) % 3) * 0.5
    if fov:
        c.cam_model[1], c.cam_w[1] = 1, 0.9
        fx, fy, u0, v0 = c.cam_params[1]
        one = c.cam == 1
        px, py = (c.z[one, 0] - u0) / fx, (c.z[one, 1] - v0) / fy
        f = scene.fov_factor(np.hypot(px, py), 0.9)
        c.z[one] = np.stack([fx * f * px + u0, fy * f * py + v0], -1)
    else:
        rng = np.random.default_rng(5)
        c.pose_cam = c.cam_params[0] * (1.0 + 0.002 * rng.standard_normal((len(c.poses), 4)))
    c.lm_active = np.ones(len(c.x_w), dtype=np.uint8)
    c.lm_active[[3, 8, 20]] = 0
    return c


@pytest.mark.parametrize("fov", (False, True), ids=("per_pose_intrinsics", "fov_camera"))
@pytest.mark.parametrize("lm_dim", (1, 3))
def test_kernel_edges(lm_dim, fov):
    c = edge_case(lm_dim, fov)
    L = len(c.x_w)
    hc = hostcheck_lib()
    host = tc.triangulate_host(hc, c)
    _, _, nfin = tc.triangulate_numpy(c)      # (the bound's V, lambda, D)
    eng = tc.engine(c)
    before = eng.get_landmarks(L)
    res, xw = eng.triangulate_landmarks(write_back=0)
    st_all = eng.triangulation_stats()
    assert np.array_equal(bits(eng.get_landmarks(L)), bits(before))
    worst = assert_matches_host(c, res, xw, host, nfin, "edges LmSize %d fov %d" % (lm_dim, fov))
    assert res[0, 0] == tc.TOO_FEW_VIEWS and res[0, 1] == 0 and res[1, 0] == tc.TOO_FEW_VIEWS and res[1, 1] == 1
    assert np.array_equal(res[:14, 1], EDGE_LENGTHS[:14])
    assert st_all["waves_early"] == 0 and st_all["written"] == 0
    n_small, n_big = track_cases.expected_ranges(EDGE_LENGTHS)
    assert st_all["waves"] == n_small + n_big
    # an id list, out of order: the same bits per landmark, and the waves without a selected landmark leave early
    ids = np.array([8, 2, 0, 60, 7, 1, 5, 9, 10], dtype=np.uint32)
    res_i, xw_i = eng.triangulate_landmarks(ids, write_back=0)
    assert np.array_equal(bits(res_i), bits(res[ids])) and np.array_equal(bits(xw_i), bits(xw[ids]))
    st = eng.triangulation_stats()
    assert st["landmarks"] == len(ids) and 0 < st["waves_early"] < st["waves"]
    # only long tracks selected: every small range leaves early
    res_b, _ = eng.triangulate_landmarks([6, 8], write_back=0)
    assert np.array_equal(bits(res_b), bits(res[[6, 8]]))
    assert eng.triangulation_stats()["waves_early"] == st["waves"] - 2
    # two identical calls return identical bits
    res2, xw2 = eng.triangulate_landmarks(write_back=0)
    assert np.array_equal(bits(res2), bits(res)) and np.array_equal(bits(xw2), bits(xw))
    print("edges, LmSize %d, fov %d: worst |dx| / bound %.3g; statuses %s" % (lm_dim, fov, worst, st_all["count"]))
    eng.close()


# ---- 5. write_back = 0 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm_dim", (1, 3))
def test_audit_changes_nothing(lm_dim):
    from ba_amd import hipapi
    c = noisy_case(16, 60, 4, 2, 0.02, lm_dim)
    L = len(c.x_w)
    masks = np.zeros(len(c.poses), dtype=np.uint16)

    def run(audit):
        eng = tc.engine(c)
        base = hipapi.device_bytes_live()
        out = None
        if audit:
            out = eng.triangulate_landmarks(write_back=0)
            again = eng.triangulate_landmarks(write_back=0)
            assert np.array_equal(bits(out[0]), bits(again[0])) and np.array_equal(bits(out[1]), bits(again[1]))
            assert hipapi.device_bytes_live() > base
            eng.release_marginals()
        assert hipapi.device_bytes_live() == base
        lms = eng.get_landmarks(L)
        eng.begin_solve()
        eng.set_pose_masks(masks)
        eng.linearize()
        S = eng.get_S()
        eng.close()
        return lms, S, out

    lms0, S0, _ = run(False)
    lms1, S1, out = run(True)
    assert np.array_equal(bits(lms0), bits(lms1)) and np.array_equal(bits(S0), bits(S1))
    assert np.array_equal(bits(lms1), bits(c.x_w))
    assert np.all(out[0][:, 0] == tc.OK) and not np.array_equal(out[1], c.x_w)     # the audit itself has results


# ---- 6. placement and refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm_dim", (1, 3))
def test_placement_and_refusals(lm_dim):
    from ba_amd import hipapi
    c = noisy_case(16, 60, 4, 2, 0.02, lm_dim)
    L, O = len(c.x_w), len(c.pose)
    masks = np.zeros(len(c.poses), dtype=np.uint16)
    eng = tc.engine(c)
    # before the first begin_solve: the next Solve sees the new coordinates
    res, xw = eng.triangulate_landmarks()
    eng.begin_solve()
    e1 = eng.eval_residuals().proj_error
    assert abs(e1 - res[:, 4].sum()) <= 1e-9 * e1
    # inside the Solve: refused, and the sentence names the way out
    with pytest.raises(hipapi.HipError, match="ba_hip_end_solve"):
        eng.triangulate_landmarks()
    eng.set_pose_masks(masks)
    eng.linearize()
    with pytest.raises(hipapi.HipError, match="ba_hip_end_solve"):
        eng.triangulate_landmarks(write_back=0)
    eng.end_solve()
    # after end_solve: served again; ba_hip_marginalize right after a writing call is refused, as after begin_solve
    eng.begin_solve()
    eng.set_pose_masks(masks)
    eng.linearize()
    eng.end_solve()
    res2, xw2 = eng.triangulate_landmarks()
    with pytest.raises(hipapi.HipError, match="needs the linearisation of the current state"):
        eng.marginalize([1])
    assert np.array_equal(bits(eng.get_landmarks(L)), bits(xw2))
    eng.begin_solve()
    e2 = eng.eval_residuals().proj_error
    assert abs(e2 - res2[:, 4].sum()) <= 1e-9 * e2
    eng.end_solve()
    # request checks on the device entry
    for kw, pattern in ((dict(ids=[1, 1]), "named twice"), (dict(ids=[L]), "is not a landmark"),
                        (dict(max_iterations=65), "max_iterations 65"), (dict(gradient_tolerance=-1.0), "negative")):
        with pytest.raises(hipapi.HipError, match=pattern):
            eng.triangulate_landmarks(**kw)
    eng.close()
    # calibration unknowns, a hooked engine, LmSize 0
    if lm_dim == 1:
        cal = tc.engine(c, finalize=False)
        cal.set_calibration(0, True)
        cal.finalize()
        with pytest.raises(hipapi.HipError, match="calibration"):
            cal.triangulate_landmarks()
        cal.close()
    hooked = tc.engine(c, finalize=False)
    hooked.set_allreduce(lambda ptr, count, dtype: 0, 0, 1)
    hooked.finalize()
    with pytest.raises(hipapi.HipError, match="sharded"):
        hooked.triangulate_landmarks()
    hooked.close()
    from helpers import _add_pose_pose
    zero = hipapi.Engine(0, 6)
    zero.set_cameras(c.cam_params, c.cam_tvs)
    zero.set_poses(c.poses)
    _add_pose_pose(zero, scene.make_scene(16, 60, 4, lm_dim=lm_dim, seed=2), len(c.poses))
    zero.finalize()
    with pytest.raises(hipapi.HipError, match="LmSize 0"):
        zero.triangulate_landmarks()
    zero.close()


# ---- 7. the class ---------------------------------------------------------------------------------------------------------
def test_class_triangulates_before_solve():
    """make_scene(14, 60, 4, LmSize 3, seed 1) with the depths off by 30 %: the start plain Gauss-Newton rejects"""
    from ba_amd import adjuster
    from helpers import fill, gn_options
    sc = scene.make_scene(14, 60, 4, lm_dim=3, seed=1, depth_sigma=0.3)
    act = np.ones(sc.num_poses, dtype=np.uint8)
    act[sc.anchor_poses] = 0
    c = tc.case_from_scene(sc, 3)
    tws, tsw = tc.tables(c)

    def reprojection_error(x_w):
        """sum |z - pi(T_sw X)|^2 over the residuals, at the uploaded poses"""
        e = 0.0
        for a in range(len(c.pose)):
            R, t = tsw[c.pose[a]][0]
            uv, _ = tc.project(tuple(c.cam_params[0]) + (0.0, 0), R @ x_w[c.lm[a], :3] + t * x_w[c.lm[a], 3])
            e += float((c.z[a] - uv) @ (c.z[a] - uv))
        return e

    codes, start = {}, {}
    for tri in (False, True):
        a = adjuster.BundleAdjuster(3, 6)
        a.Init(gn_options(adjuster))
        fill(a, sc, active=act)
        if tri:
            ok, res = a.TriangulateLandmarks()
            assert ok and res.shape == (sc.num_landmarks, 8)
            print("statuses of the class call:", np.bincount(res[:, 0].astype(int), minlength=6))
            lms = a.landmarks()
            assert np.array_equal(bits(lms), bits(a.engine_landmarks()))
            assert not np.array_equal(lms, sc.landmarks)
        start[tri] = reprojection_error(a.landmarks())
        a.Solve(1)
        codes[tri] = adjuster.RESULT_NAMES[a.summary().result]
    print("first Gauss-Newton step without / with triangulation: %s / %s; starting error %.6g / %.6g"
          % (codes[False], codes[True], start[False], start[True]))
    assert start[True] < start[False]
