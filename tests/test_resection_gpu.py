"""Pose refinement (resection) with the landmarks held fixed on the device (ba_hip_refine_poses, k_resect.hip): against
the host restatement of the same rules at the observation counts where the kernel changes its path, against the kernels
that existed before it (residual evaluation and linearisation at the poses it wrote), and in its effects on the engine."""
import functools

import numpy as np
import pytest

import resection_cases as rc
import triangulation_cases as tc
from ba_amd import scene
from helpers import hostcheck_lib

pytestmark = pytest.mark.gpu
EPS = rc.EPS
STEP_TOL = rc.DEFAULTS["step_tolerance"]
ROUNDING = ("an accept / reject or stop decision within rounding of its threshold moves the count by one: look at the "
            "gain ratio and c of the pose before anything else")
EDGE_VARIANTS = {"plain3": (3, dict()), "plain1": (1, dict()), "rig1": (1, dict(rig=True)), "rig3": (3, dict(rig=True)),
                 "fov3": (3, dict(fov=True)), "pose_cam1": (1, dict(pose_cam=True)),
                 "outliers3": (3, dict(outlier_frac=0.02, direction=True)),
                 "huber1": (1, dict(rig=True, outlier_frac=0.02))}
EDGE_OPTIONS = {"huber1": dict(huber_width=2.0)}   # every other variant at the defaults


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """the edge counts with half a pixel of noise, poses off by 0.1 m / 3 degrees; and the host restatement at the
    defaults, computed once and left unchanged"""
    lm_dim, kw = EDGE_VARIANTS[name]
    c, _ = rc.make_case(rc.EDGE_COUNTS, lm_dim, seed=11, pixel_sigma=0.5, **kw)
    s = rc.perturbed(c)
    return s, rc.refine_host(hostcheck_lib(), s, EDGE_OPTIONS.get(name))


def assert_matches_host(s, dev, host, what, ids=None):
    """statuses, used / excluded and iteration counts equal the host restatement's; refined poses within
    2 step_tolerance s + 8 cond2(H + lambda D) eps s (H, lambda of the restatement's end point), info36 within
    8 k eps |H|_max, the others bit for bit as they were.  Returns the worst ratios (pose, information)."""
    res, t7, info = dev
    hres, ht7, hinfo, hfin = host
    for col in (0, 1, 7):
        assert np.array_equal(res[:, col], hres[:, col]), (what, col, res[:, col], hres[:, col])
    differ = np.nonzero(res[:, 2] != hres[:, 2])[0]
    assert len(differ) == 0, "%s: iteration counts differ on rows %s (device %s, host %s); %s" % (
        what, differ, res[differ, 2], hres[differ, 2], ROUNDING)
    worst, worst_h = 0.0, 0.0
    for row in range(len(res)):
        p = row if ids is None else ids[row]
        if res[row, 0] in (rc.OK, rc.NOT_CONVERGED):
            bt, br = rc.pose_bounds(hinfo[row], hfin[row, 0], ht7[row, :3], STEP_TOL)
            et = np.linalg.norm(t7[row, :3] - ht7[row, :3]) / bt
            er = rc.angle_between(t7[row, 3:], ht7[row, 3:]) / br
            eh = np.abs(info[row] - hinfo[row]).max() / (8.0 * res[row, 1] * EPS * np.abs(hinfo[row]).max())
            worst, worst_h = max(worst, et, er), max(worst_h, eh)
            assert et <= 1.0 and er <= 1.0 and eh <= 1.0, (what, p, et, er, eh)
            assert np.array_equal(info[row], info[row].T)
        else:
            assert np.array_equal(bits(t7[row]), bits(s.poses[p])) and not info[row].any(), (what, p)
    return worst, worst_h


# ---- 1. device against the host restatement at the edge counts ---------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EDGE_VARIANTS))
def test_device_matches_host_restatement(name):
    """Every edge count, both landmark sizes, rig / FOV / per-pose intrinsics / outliers, at the defaults; huber1 with a
    Huber width of 2 pixels on the rig with outliers.  There the pose of 1 100 observations ends NOT_CONVERGED in the host
    restatement and in the numpy LM alike: with recomputed weights E = sum w(r) |r|^2 and g = sum w J^T r belong to
    different costs, every step is rejected from c = 1.6e-5 on and lambda runs to its ceiling; the pose is written, its
    cost fell.
    Measured on one MI355X when the test was written: worst pose ratio 3.4e-5, worst information ratio 0.11.  The pose
    of 3 observations is exactly determined: its cost falls to 1e-27 and the refinement ends by E <= F (resect.h) after
    8 iterations on the device and on the host; before that rule the device took 14 and the host 9, both deciding on
    rounding noise below the floor."""
    s, host = edge_case(name)
    P = len(s.poses)
    eng = rc.engine(s)
    before = eng.get_poses(P)[0]
    opts = EDGE_OPTIONS.get(name, {})
    dev = eng.refine_poses(write_back=0, **opts)
    assert np.array_equal(bits(eng.get_poses(P)[0]), bits(before))
    worst, worst_h = assert_matches_host(s, dev, host, name)
    res = dev[0]
    assert np.array_equal(res[:, 1] + res[:, 7], rc.EDGE_COUNTS)
    assert np.all(res[:3, 0] == rc.TOO_FEW) and np.all(np.isin(res[3:, 0], (rc.OK, rc.NOT_CONVERGED)))
    assert np.all(res[3:, 4] < res[3:, 3])
    if not opts:      # (huber1: the pose of 1 100 observations stalls at c = 1.6e-5, see the docstring)
        assert np.all(res[4:, 0] == rc.OK)
    st = eng.pose_refinement_stats()
    assert st["poses"] == P and st["written"] == 0 and st["count"]["TOO_FEW_OBSERVATIONS"] == 3
    assert st["observations_used"] == res[:, 1].sum() and st["observations_excluded"] == res[:, 7].sum()
    if name in ("outliers3", "huber1"):
        assert res[:, 7].sum() > 0
    # an id list, out of order, across the three kernels: the same bits per pose; and two calls give identical bits
    ids = np.array([12, 0, 7, 3, 10, 5, 11], dtype=np.uint32)
    part = eng.refine_poses(ids, write_back=0, **opts)
    again = eng.refine_poses(write_back=0, **opts)
    for a, b, c_ in zip(dev, part, again):
        assert np.array_equal(bits(a[ids]), bits(b)) and np.array_equal(bits(a), bits(c_))
    print("device against host, %s: worst pose ratio %.3g, information ratio %.3g, %.3f ms; statuses %s"
          % (name, worst, worst_h, st["device_ms"], st["count"]))   # (the last call's time)
    eng.close()


# ---- 2. the result satisfies the kernels that exist without the feature -------------------------------------------------
@functools.lru_cache(maxsize=None)
def clean_case(lm_dim):
    """no excluded observations, and no pose of fewer than 3: every requested pose is written"""
    c, _ = rc.make_case((3, 63, 64, 65, 255, 256, 257, 1024, 1025, 1100), lm_dim, seed=12, pixel_sigma=0.5)
    return rc.perturbed(c)


def longdouble_cost(s, poses):
    """sum w |z - pi(P)|^2 at the poses in numpy.longdouble (pinhole, T_vs the identity): the reference for the roundings
    of a cost evaluation"""
    ld = np.longdouble
    total = ld(0)
    fx, fy, u0, v0 = (ld(v) for v in s.cam_params[0])
    for p in range(len(poses)):
        a = np.nonzero(s.pose == p)[0]
        x, y, z, w = (ld(v) for v in poses[p, 3:7])
        n = np.sqrt(x * x + y * y + z * z + w * w)
        x, y, z, w = x / n, y / n, z / n, w / n
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=ld)
        X = s.x_w[s.lm[a]].astype(ld)
        Pp = (X[:, :3] - X[:, 3:4] * poses[p, :3].astype(ld)) @ R
        r0 = s.z[a, 0].astype(ld) - (fx * Pp[:, 0] / Pp[:, 2] + u0)
        r1 = s.z[a, 1].astype(ld) - (fy * Pp[:, 1] / Pp[:, 2] + v0)
        total += np.sum(s.weight[a].astype(ld) * (r0 * r0 + r1 * r1))
    return total


@pytest.mark.parametrize("lm_dim", (1, 3))
def test_result_satisfies_existing_kernels(lm_dim):
    """After a write-back of all poses, ba_hip_eval_residuals gives the sum of the final costs to (O + 16) 2^-53 relative
    (all terms positive: any summation order); with LmSize 1 the re-derived x_s adds roundings that count does not cover,
    so the bound grows by 8 x the relative distance of the host restatement's sum from a numpy.longdouble evaluation at
    the same poses (the margin test_step_path_gpu.py takes over its oracle).  With LmSize 3 the linearisation's own
    Jacobians give, per pose, |sum w j_meas^T r|_i / sqrt(H_ii E_p) <= gradient_tolerance + 4 k eps."""
    s = clean_case(lm_dim)
    P, O = len(s.poses), len(s.pose)
    eng = rc.engine(s)
    res, t7, _ = eng.refine_poses()
    assert np.all(res[:, 0] <= rc.NOT_CONVERGED) and np.all(res[:, 7] == 0) and np.all(res[1:, 0] == rc.OK)
    assert eng.pose_refinement_stats()["written"] == P
    assert np.array_equal(bits(eng.get_poses(P)[0]), bits(t7))
    total = float(res[:, 4].sum())
    tol = (O + 16) * 2.0 ** -53
    if lm_dim == 1:
        hres, ht7 = rc.refine_host(hostcheck_lib(), s)[:2]
        ref = longdouble_cost(s, ht7)
        measured = float(abs(np.longdouble(hres[:, 4].sum()) - ref) / ref)
        print("host restatement against longdouble at the same poses: %.3g relative" % measured)
        tol += 8.0 * measured
    eng.begin_solve()
    ev = eng.eval_residuals()
    figure = abs(ev.proj_error - total) / total / tol
    print("LmSize %d: proj_error %.17g, sum of costs %.17g, |difference| / (total tol) = %.3g" % (lm_dim, ev.proj_error, total, figure))
    assert figure <= 1.0
    if lm_dim == 3:
        eng.set_pose_masks(np.zeros(P, dtype=np.uint16))
        eng.linearize()
        jm, _, _, r = eng.get_proj_jacobians(O)
        worst = 0.0
        for p in range(1, P):           # (pose 0 is inactive in the joint problem: no Jacobian block)
            a = np.nonzero(s.pose == p)[0]
            J, rr = jm[a].reshape(-1, 6), r[a].reshape(-1)
            cg = np.max(np.abs(J.T @ rr) / np.sqrt(np.sum(J * J, axis=0) * (rr @ rr)))
            lim = rc.DEFAULTS["gradient_tolerance"] + 4 * len(a) * EPS
            worst = max(worst, cg / lim)
            assert cg <= lim, (p, cg, lim, res[p])
        print("worst gradient ratio %.3g" % worst)
    eng.close()


# ---- 3. write_back = 0 changes nothing held -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def window_case(lm_dim):
    sc = scene.make_scene(14, 60, 4, lm_dim=lm_dim, seed=2)
    return tc.case_from_scene(sc, lm_dim)


@pytest.mark.parametrize("lm_dim", (1, 3))
def test_audit_changes_nothing(lm_dim):
    from ba_amd import hipapi
    c = window_case(lm_dim)
    P, L = len(c.poses), len(c.x_w)
    eng = tc.engine(c)
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(P, dtype=np.uint16))
    eng.linearize()
    eng.solve_gn()
    eng.end_solve()
    B = np.linspace(-1.0, 1.0, eng.num_pose_params())
    held = lambda: (eng.get_poses(P), eng.get_landmarks(L), eng.factor_solve(B))
    (poses0, v0, b0), lms0, x0 = held()
    base = hipapi.device_bytes_live()
    out = eng.refine_poses(write_back=0)
    again = eng.refine_poses(write_back=0)
    assert hipapi.device_bytes_live() > base
    for a, b in zip(out, again):
        assert np.array_equal(bits(a), bits(b))
    (poses1, v1, b1), lms1, x1 = held()
    for a, b in ((poses0, poses1), (v0, v1), (b0, b1), (lms0, lms1), (x0, x1)):
        assert np.array_equal(bits(a), bits(b))
    assert np.all(out[0][:, 0] <= rc.NOT_CONVERGED) and not np.array_equal(out[1], poses0)   # the audit has results
    # after ba_hip_release_marginals the work space is rebuilt and gives the same bits (before the Solve below: with
    # LmSize 1 an end_solve re-derives x_w from x_s, which moves the landmarks by a rounding)
    eng.release_marginals()
    assert hipapi.device_bytes_live() <= base
    rebuilt = eng.refine_poses(write_back=0)
    for a, b in zip(out, rebuilt):
        assert np.array_equal(bits(a), bits(b))
    eng.begin_solve()
    e1 = eng.eval_residuals().proj_error
    eng.end_solve()
    # the same calls on a second engine, without the audit
    ref = tc.engine(c)
    ref.begin_solve()
    ref.set_pose_masks(np.zeros(P, dtype=np.uint16))
    ref.linearize()
    ref.solve_gn()
    ref.end_solve()
    ref.begin_solve()
    e0 = ref.eval_residuals().proj_error
    ref.close()
    assert e0 == e1
    eng.close()


# ---- 4. what a writing call leaves bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("lm_dim", (1, 3))
def test_untouched_state_stays_bitwise(lm_dim):
    s, host = edge_case("plain%d" % lm_dim)
    P, L = len(s.poses), len(s.x_w)
    rng = np.random.default_rng(3)
    v_w, b = rng.normal(size=(P, 3)), 0.01 * rng.normal(size=(P, 6))
    eng = rc.engine(s, pose_dim=15, v_w=v_w, b=b)
    lms = eng.get_landmarks(L)
    ids = np.array([1, 2, 3, 6, 9, 12], dtype=np.uint32)     # 1, 2: TOO_FEW; the others across the three kernels
    res, t7, _ = eng.refine_poses(ids)
    assert list(res[:, 0]) == [rc.TOO_FEW, rc.TOO_FEW] + list(host[0][ids[2:], 0])
    assert eng.pose_refinement_stats()["written"] == 4
    poses, v1, b1 = eng.get_poses(P)
    rest = np.setdiff1d(np.arange(P), ids[2:])
    assert np.array_equal(bits(poses[rest]), bits(s.poses[rest]))          # not requested, or TOO_FEW
    assert np.array_equal(bits(poses[ids]), bits(t7)) and not np.array_equal(poses[ids[2:]], s.poses[ids[2:]])
    assert np.array_equal(bits(v1), bits(v_w)) and np.array_equal(bits(b1), bits(b))
    assert np.array_equal(bits(eng.get_landmarks(L)), bits(lms)) and np.array_equal(bits(lms), bits(s.x_w))
    eng.close()
    # FAILED: a finite pose with a NaN pixel (used: its point is fine; the starting cost is not finite), on poses of 3,
    # 65 and 1 100 observations, one per kernel path and the smallest that is refined; TOO_FEW exactly: a pose that is
    # itself not finite has no usable observation.  A writing call leaves all of them bit for bit, their neighbours OK.
    bad = s.copy()
    for p in (3, 6, 12):
        bad.z[np.nonzero(bad.pose == p)[0][1], 1] = np.nan
    bad.poses[9, 1] = np.nan
    hres, ht7, hinfo, _ = rc.refine_host(hostcheck_lib(), bad)
    eng = rc.engine(bad)
    ids = np.array([3, 4, 6, 7, 9, 11, 12], dtype=np.uint32)
    res, t7, info = eng.refine_poses(ids)
    assert list(res[:, 0]) == [rc.FAILED, rc.OK, rc.FAILED, rc.OK, rc.TOO_FEW, rc.OK, rc.FAILED]
    assert np.array_equal(res[:, 0], hres[ids, 0]) and np.array_equal(res[:, [1, 2, 7]], hres[ids][:, [1, 2, 7]])
    failed = np.array([0, 2, 6])
    assert np.array_equal(res[failed, 1], [3, 65, 1100]) and not res[failed, 2:5].any() and not res[failed, 6:].any()
    assert not info[failed].any() and not info[4].any() and res[4, 1] == 0 and res[4, 7] == rc.EDGE_COUNTS[9]
    st = eng.pose_refinement_stats()
    assert st["count"] == {"OK": 3, "NOT_CONVERGED": 0, "TOO_FEW_OBSERVATIONS": 1, "FAILED": 3} and st["written"] == 3
    poses = eng.get_poses(P)[0]
    for p in (3, 6, 9, 12):
        assert np.array_equal(bits(poses[p]), bits(bad.poses[p]))
        assert np.array_equal(bits(t7[list(ids).index(p)]), bits(bad.poses[p]))
    assert np.array_equal(bits(poses[ids]), bits(t7)) and not np.array_equal(poses[[4, 7, 11]], bad.poses[[4, 7, 11]])
    eng.close()


def test_fixed_mask_on_the_device():
    s, _ = edge_case("plain3")
    P = len(s.poses)
    host = rc.refine_host(hostcheck_lib(), s, dict(fixed_mask=0b111000))
    eng = rc.engine(s)
    dev = eng.refine_poses(fixed_mask=0b111000)
    assert_matches_host(s, dev, host, "rotation fixed")
    poses = eng.get_poses(P)[0]
    assert np.array_equal(bits(poses[:, 3:]), bits(s.poses[:, 3:])) and not np.array_equal(poses[4:, :3], s.poses[4:, :3])
    eng.close()


# ---- 5. placement and refusals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm_dim", (1, 3))
def test_placement_and_refusals(lm_dim):
    from ba_amd import hipapi
    c = window_case(lm_dim)
    P = len(c.poses)
    masks = np.zeros(P, dtype=np.uint16)
    eng = tc.engine(c)
    # before the first begin_solve: the next Solve sees the new poses
    res, t7, _ = eng.refine_poses()
    eng.begin_solve()
    e1 = eng.eval_residuals().proj_error
    assert abs(e1 - res[:, 4].sum()) <= 1e-9 * e1
    # inside the Solve: refused, and the sentence names the way out
    with pytest.raises(hipapi.HipError, match="ba_hip_end_solve"):
        eng.refine_poses()
    eng.set_pose_masks(masks)
    eng.linearize()
    with pytest.raises(hipapi.HipError, match="ba_hip_end_solve"):
        eng.refine_poses(write_back=0)
    eng.end_solve()
    # after end_solve: served again; a writing call counts as a begin_solve for the linearisation held
    eng.begin_solve()
    eng.set_pose_masks(masks)
    eng.linearize()
    eng.end_solve()
    res2, t72, _ = eng.refine_poses()
    with pytest.raises(hipapi.HipError, match="needs the linearisation of the current state"):
        eng.marginalize([1])
    assert np.array_equal(bits(eng.get_poses(P)[0]), bits(t72))
    for kw, pattern in ((dict(ids=[1, 1]), "named twice"), (dict(ids=[P]), "is not a pose"), (dict(ids=[]), "no pose requested"),
                        (dict(max_iterations=65), "max_iterations 65"), (dict(gradient_tolerance=-1.0), "negative"),
                        (dict(fixed_mask=63), "fixed_mask 63")):
        with pytest.raises(hipapi.HipError, match=pattern):
            eng.refine_poses(**kw)
    eng.close()
    hooked = tc.engine(c, finalize=False)
    hooked.set_allreduce(lambda ptr, count, dtype: 0, 0, 1)
    hooked.finalize()
    with pytest.raises(hipapi.HipError, match="sharded"):
        hooked.refine_poses()
    hooked.close()
    fresh = tc.engine(c, finalize=False)
    with pytest.raises(hipapi.HipError, match="ba_hip_finalize"):
        fresh.refine_poses()
    fresh.close()


# ---- 6. the class ------------------------------------------------------------------------------------------------------------
def test_class_refines_before_a_solve():
    """make_scene(14, 60, 4) with the landmarks at ground truth and every pose but the anchors off by 0.1 m / 3 degrees:
    RefinePoses, then Solve(1), against Solve(1) alone.  Asserted: the statuses are the host restatement's and the refined
    cost is below the starting cost; the outcome of the joint step is printed, not asserted."""
    from ba_amd import adjuster
    from helpers import fill, gn_options
    sc = scene.make_scene(14, 60, 4, lm_dim=3, seed=1, depth_sigma=0.0, trans_sigma=0.0, rot_sigma=0.0)
    sc.landmarks = sc.gt_landmarks.copy()
    act = np.ones(sc.num_poses, dtype=np.uint8)
    act[sc.anchor_poses] = 0
    c = tc.case_from_scene(sc, 3)
    moved = rc.perturbed(c, seed=9)
    moved.poses[sc.anchor_poses] = c.poses[sc.anchor_poses]
    sc.poses = moved.poses.copy()
    c = tc.case_from_scene(sc, 3)
    hres, ht7 = rc.refine_host(hostcheck_lib(), c)[:2]
    codes, errors = {}, {}
    for refine in (False, True):
        a = adjuster.BundleAdjuster(3, 6)
        a.Init(gn_options(adjuster))
        fill(a, sc, active=act)
        if refine:
            ok, res, t7, info = a.RefinePoses()
            assert ok and res.shape == (sc.num_poses, 8) and info.shape == (sc.num_poses, 6, 6)
            assert np.array_equal(res[:, 0], hres[:, 0]) and np.array_equal(res[:, 1], hres[:, 1])
            assert res[:, 4].sum() < res[:, 3].sum()
            assert np.array_equal(bits(a.poses()[0]), bits(t7))
            errors["refined"] = (res[:, 3].sum(), res[:, 4].sum())
            print("statuses of the class call:", np.bincount(res[:, 0].astype(int), minlength=4))
        a.Solve(1)
        codes[refine] = adjuster.RESULT_NAMES[a.summary().result]
    print("first Gauss-Newton step without / with RefinePoses: %s / %s; projection cost before / after the call %.6g / %.6g"
          % (codes[False], codes[True], errors["refined"][0], errors["refined"][1]))
