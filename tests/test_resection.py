"""Pose refinement (resection) with the landmarks held fixed, on the CPU: the per-pose list builder and the rules of
ba_amd/csrc/resect.h through the host restatement ba_hostcheck_refine_poses (the functions the kernel of k_resect.hip
applies), against ground truth and against the independent numpy LM of tests/resection_cases.py."""
import ctypes

import numpy as np
import pytest

import lifecycle_cases as lc
import resection_cases as rc
from helpers import hostcheck_lib

EPS = rc.EPS
VARIANTS = {"plain": dict(), "rig": dict(rig=True), "fov": dict(fov=True), "pose_cam": dict(pose_cam=True),
            "direction": dict(direction=True)}


@pytest.fixture(scope="module")
def hc():
    return hostcheck_lib()


def _lists(hc, P, obs_pose):
    obs_pose = np.ascontiguousarray(obs_pose, dtype=np.uint32)
    ptr, idx = np.zeros(P + 1, dtype=np.uint32), np.zeros(max(len(obs_pose), 1), dtype=np.uint32)
    U32 = ctypes.c_uint32
    rcode = hc.ba_hostcheck_pose_obs_lists(U32(P), U32(len(obs_pose)), rc.tc._ptr(obs_pose, U32), rc.tc._ptr(ptr, U32),
                                           rc.tc._ptr(idx, U32))
    return rcode, ptr, idx[:len(obs_pose)]


# ---- 1. the list builder ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,O,seed", [(1, 0, 0), (1, 7, 1), (5, 0, 2), (9, 300, 3), (40, 33, 4), (13, 4200, 5)])
def test_pose_lists_match_argsort(hc, P, O, seed):
    """CSR over all poses by id, entries ascending positions of the sorted observation order: numpy's stable argsort by
    pose.  (40, 33) leaves poses without observations, P = 1 has one list."""
    rng = np.random.default_rng(seed)
    obs_pose = rng.integers(0, P, size=O).astype(np.uint32)
    if P == 9:
        obs_pose[obs_pose == 4] = 5   # a pose without observations between others
    rcode, ptr, idx = _lists(hc, P, obs_pose)
    assert rcode == 0
    want_ptr = np.zeros(P + 1, dtype=np.uint32)
    np.cumsum(np.bincount(obs_pose, minlength=P), out=want_ptr[1:])
    assert np.array_equal(ptr, want_ptr)
    assert np.array_equal(idx, np.argsort(obs_pose, kind="stable"))
    for p in range(P):
        assert np.all(np.diff(idx[ptr[p]:ptr[p + 1]].astype(np.int64)) > 0)


def test_pose_lists_on_a_case_and_out_of_range(hc):
    c, _ = rc.make_case(rc.SMALL_COUNTS, 3, seed=2)
    rcode, ptr, idx = _lists(hc, len(c.poses), c.pose[rc.sorted_order(c)])
    want_ptr, want_idx = rc.pose_lists(c)
    assert rcode == 0 and np.array_equal(ptr, want_ptr) and np.array_equal(idx, want_idx)
    assert list(np.diff(ptr.astype(np.int64))) == list(rc.SMALL_COUNTS)
    assert _lists(hc, 3, [0, 1, 3])[0] == 1


# ---- 2. noise-free data: the truth comes back --------------------------------------------------------------------------
@pytest.mark.parametrize("lm_dim", (1, 3))
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_noise_free_poses_are_recovered(hc, variant, lm_dim):
    """True pixels, true landmarks, poses off by 0.1 m / 3 degrees: every pose with at least 40 observations comes back to
    8 cond2(H) eps (|t| + 1) in translation and 8 cond2(H) eps in the angle of q^-1 q_true, H the information the call
    returns.  Poses of 3 observations are exactly determined but three points admit several poses, so they are not held
    to the truth; below 3 the status is TOO_FEW_OBSERVATIONS and the pose comes back bit for bit.
    Measured when the test was written: worst ratio to the bound 1.2e-3 (cond2(H) 3.9e3 .. 6.1e3; the refinement ends by
    E <= F, the cost's rounding floor)."""
    c, true = rc.make_case(rc.SMALL_COUNTS, lm_dim, seed=3, **VARIANTS[variant])
    s = rc.perturbed(c)
    res, t7, info, _ = rc.refine_host(hc, s)
    worst = 0.0
    for p, k in enumerate(rc.SMALL_COUNTS):
        assert res[p, 1] == k and res[p, 7] == 0
        if k < 3:
            assert res[p, 0] == rc.TOO_FEW and np.array_equal(t7[p], s.poses[p]) and not info[p].any()
            continue
        assert res[p, 0] in (rc.OK, rc.NOT_CONVERGED) and res[p, 4] < res[p, 3]
        assert np.array_equal(info[p], info[p].T)
        if k < 40:
            continue
        cond = np.linalg.cond(info[p])
        et = np.linalg.norm(t7[p, :3] - true[p, :3]) / (8.0 * cond * EPS * (np.linalg.norm(true[p, :3]) + 1.0))
        er = rc.angle_between(t7[p, 3:], true[p, 3:]) / (8.0 * cond * EPS)
        worst = max(worst, et, er)
        assert et <= 1.0 and er <= 1.0, (p, et, er, cond)
    print("worst ratio to the bound", worst)


# ---- 3. against the independent numpy LM -------------------------------------------------------------------------------
def _agree(hc, s, opts, wrong=None, ids=None):
    """the worst ratio of |host - numpy| to the bound over the refined poses, and whether statuses and counts agree"""
    st = opts.get("step_tolerance", 1e-12)
    rh = rc.refine_host(hc, s, opts, ids)
    rn = rc.refine_numpy(s, opts, ids, wrong=wrong)
    same = np.array_equal(rh[0][:, 0], rn[0][:, 0]) and np.array_equal(rh[0][:, 1], rn[0][:, 1]) and \
        np.array_equal(rh[0][:, 7], rn[0][:, 7])
    worst = 0.0
    for row in range(len(rh[0])):
        if rh[0][row, 0] not in (rc.OK, rc.NOT_CONVERGED):
            assert np.array_equal(rh[1][row], s.poses[row if ids is None else ids[row]])
            continue
        bt, br = rc.pose_bounds(rh[2][row], rh[3][row, 0], rh[1][row, :3], st, opts.get("fixed_mask", 0))
        worst = max(worst, np.linalg.norm(rh[1][row, :3] - rn[1][row, :3]) / bt,
                    rc.angle_between(rh[1][row, 3:], rn[1][row, 3:]) / br)
    return worst, same


NOISY = {"plain3": (3, dict(), dict()), "rig1": (1, dict(rig=True), dict()), "fov3": (3, dict(fov=True), dict()),
         "pose_cam1": (1, dict(pose_cam=True), dict()), "direction1": (1, dict(direction=True), dict()),
         "outliers3": (3, dict(outlier_frac=0.02), dict(huber_width=2.0)),
         "outliers_rig1": (1, dict(rig=True, outlier_frac=0.02), dict(huber_width=2.0)),
         "masked3": (3, dict(), dict(fixed_mask=0b100010))}


@pytest.mark.parametrize("name", sorted(NOISY))
def test_host_restatement_meets_numpy(hc, name):
    """Half a pixel of noise, step_tolerance 1e-9: the two CPU implementations end within
    2 step_tolerance s + 8 cond2(H + lambda D) eps s of each other (s = |t| + 1 for the translation, 1 for the rotation),
    with equal statuses, used and excluded counts.  Measured when the test was written: worst ratio 1.1e-6."""
    lm_dim, kw, o = NOISY[name]
    c, _ = rc.make_case(rc.SMALL_COUNTS, lm_dim, seed=4, pixel_sigma=0.5, **kw)
    s = rc.perturbed(c)
    worst, same = _agree(hc, s, dict(step_tolerance=1e-9, **o))
    print(name, "worst ratio", worst)
    assert same and worst <= 1.0


def test_edge_counts_meet_numpy(hc):
    """the kernel's edge counts (0 .. 3, the wave, the block, 1 024 / 1 025, 1 100) through both CPU implementations"""
    c, _ = rc.make_case(rc.EDGE_COUNTS, 3, seed=6, pixel_sigma=0.5)
    worst, same = _agree(hc, rc.perturbed(c), dict(step_tolerance=1e-9))
    assert same and worst <= 1.0


def test_excluded_observations_are_counted(hc):
    c, _ = rc.make_case(rc.SMALL_COUNTS, 3, seed=4, pixel_sigma=0.5, outlier_frac=0.05)
    s = rc.perturbed(c)
    res = rc.refine_host(hc, s, dict(huber_width=2.0))[0]
    ref = rc.refine_numpy(s, dict(huber_width=2.0))[0]
    assert res[:, 7].sum() > 0 and np.array_equal(res[:, 7], ref[:, 7])
    assert np.array_equal(res[:, 1] + res[:, 7], rc.SMALL_COUNTS)
    assert np.all(res[res[:, 1] > 0, 5] > 0)     # the smallest depth is over the used observations


def _nan_pixel(s, pose):
    """the case with one pixel coordinate of one observation of `pose` made NaN: a finite pose, a non-finite cost"""
    bad = s.copy()
    a = np.nonzero(bad.pose == pose)[0][1]
    bad.z[a, 1] = np.nan
    return bad


@pytest.mark.parametrize("lm_dim", (1, 3))
def test_non_finite_cost_is_failed(hc, lm_dim):
    """A NaN pixel on poses of 3 and of 65 observations: the point is finite and in front, so the observation is used,
    the starting cost is not finite and the status is FAILED exactly, in the restatement and in the numpy LM: pose bit
    for bit, zero cost columns, zero information, no iteration; the other poses are refined as without it.  A pose that
    is itself not finite has no usable observation: TOO_FEW_OBSERVATIONS exactly, all of its observations excluded."""
    c, _ = rc.make_case(rc.SMALL_COUNTS, lm_dim, seed=4, pixel_sigma=0.5)
    s = rc.perturbed(c)
    bad = _nan_pixel(_nan_pixel(s, 2), 4)
    bad.poses[5, 1] = np.nan
    res, t7, info, final = rc.refine_host(hc, bad)
    ref = rc.refine_numpy(bad)[0]
    clean = rc.refine_host(hc, s)
    assert list(res[:, 0]) == [rc.TOO_FEW, rc.TOO_FEW, rc.FAILED, rc.OK, rc.FAILED, rc.TOO_FEW]
    for col in (0, 1, 7):
        assert np.array_equal(res[:, col], ref[:, col])
    for p in (2, 4):
        assert res[p, 1] == rc.SMALL_COUNTS[p] and res[p, 7] == 0      # used: the point itself is fine
        assert not res[p, 2:5].any() and res[p, 6] == 0 and not info[p].any()
        assert np.array_equal(t7[p].view(np.uint64), bad.poses[p].view(np.uint64))
    assert res[5, 1] == 0 and res[5, 7] == rc.SMALL_COUNTS[5]
    assert np.array_equal(t7[5].view(np.uint64), bad.poses[5].view(np.uint64))
    for a, b in zip((res, t7, info), clean[:3]):
        assert np.array_equal(a[3], b[3])


# ---- 4. fixed_mask -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", (0b000111, 0b111000, 0b000001, 0b010000, 0b111110))
def test_fixed_parameters_stay_bitwise(hc, mask):
    c, _ = rc.make_case(rc.SMALL_COUNTS, 3, seed=7, pixel_sigma=0.3)
    s = rc.perturbed(c)
    res, t7, info, final = rc.refine_host(hc, s, dict(fixed_mask=mask))
    ran = np.isin(res[:, 0], (rc.OK, rc.NOT_CONVERGED))
    assert ran[3:].all() and np.any(t7[ran] != s.poses[ran])
    for i in range(3):
        if mask >> i & 1:
            assert np.array_equal(t7[:, i], s.poses[:, i])
    if mask & 0b111000 == 0b111000:
        assert np.array_equal(t7[:, 3:], s.poses[:, 3:])
    for i in range(6):
        if mask >> i & 1:
            assert not info[:, i, :].any() and not info[:, :, i].any() and not final[:, 1 + i].any()
    # TOO_FEW counts the free parameters: 2 observations serve up to 4 of them
    free = 6 - bin(mask).count("1")
    assert (res[1, 0] == rc.TOO_FEW) == (2 * rc.SMALL_COUNTS[1] < free)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def _guard(hc, events, lm_dim=3, flags=0):
    ev = np.array([lc.EVENTS.index(e) for e in events], dtype=np.int32)
    msg = ctypes.create_string_buffer(512)
    rcode = hc.ba_hostcheck_refine_poses_guard(ctypes.c_uint32(len(ev)), rc.tc._ptr(ev, ctypes.c_int32), lm_dim,
                                               ctypes.c_uint32(flags), msg, ctypes.c_uint32(512))
    assert rcode in (0, 1)
    return msg.value.decode()


def test_guard_refusals(hc):
    who = "ba_hip_refine_poses: "
    assert _guard(hc, ()) == who + lc.NOT_FINALIZED
    assert _guard(hc, lc.FINALIZE) == ""
    assert _guard(hc, lc.FINALIZE + ("solve_begins",)) == ""          # (in_solve is the engine's flag, not the record's)
    assert "LmSize 0" in _guard(hc, lc.FINALIZE, lm_dim=0)
    assert "calibration" in _guard(hc, lc.FINALIZE, flags=1)
    for f in (2, 8, 16):
        assert "sharded" in _guard(hc, lc.FINALIZE, flags=f)
    assert "inside a Solve" in _guard(hc, lc.FINALIZE, flags=4)
    assert "LmSize 0" in _guard(hc, lc.FINALIZE, lm_dim=0, flags=1 | 4)   # first refusal first


def test_request_refusals(hc):
    c, _ = rc.make_case((5, 6), 3, seed=1)
    assert "max_iterations 65" in rc.refine_host(hc, c, dict(max_iterations=65))
    assert "max_iterations -1" in rc.refine_host(hc, c, dict(max_iterations=-1))
    for k in ("initial_damping", "gradient_tolerance", "step_tolerance", "huber_width"):
        assert "must not be negative" in rc.refine_host(hc, c, {k: -1e-3})
        assert "must not be negative" in rc.refine_host(hc, c, {k: np.nan})
    assert "fixed_mask 63" in rc.refine_host(hc, c, dict(fixed_mask=63))
    assert "fixed_mask 64" in rc.refine_host(hc, c, dict(fixed_mask=64))
    assert "id 2 is not a pose" in rc.refine_host(hc, c, ids=[0, 2])
    assert "pose 1 is named twice" in rc.refine_host(hc, c, ids=[1, 0, 1])
    assert "no pose requested" in rc.refine_host(hc, c, ids=[])
    assert not isinstance(rc.refine_host(hc, c, dict(max_iterations=0, fixed_mask=62), ids=[1]), str)


def test_ids_select_rows_in_request_order(hc):
    c, _ = rc.make_case(rc.SMALL_COUNTS, 3, seed=4, pixel_sigma=0.5)
    s = rc.perturbed(c)
    full = rc.refine_host(hc, s)
    part = rc.refine_host(hc, s, ids=[5, 0, 3])
    for a, b in zip(full, part):
        assert np.array_equal(a[[5, 0, 3]], b)


# ---- 6. the comparison can tell: wrong restatements ---------------------------------------------------------------------
def _wrong_case(wrong):
    if wrong == "no_trial_cheirality":
        return rc.cheirality_trap()[0], dict(step_tolerance=1e-9)
    lm_dim, kw, o = {"rotation_side": (3, dict(), dict()), "no_tvs": (3, dict(rig=True), dict()),
                     "drop_same_pose": (1, dict(), dict()),
                     "huber_frozen": (3, dict(outlier_frac=0.05), dict(huber_width=2.0))}[wrong]
    c, _ = rc.make_case(rc.SMALL_COUNTS, lm_dim, seed=4, pixel_sigma=0.5, **kw)
    return rc.perturbed(c), dict(step_tolerance=1e-9, **o)


@pytest.mark.parametrize("wrong", rc.WRONG)
def test_wrong_restatements_are_told(hc, wrong):
    """Each deliberate mistake in the numpy LM — the rotation update on the wrong side, T_vs ignored, same-pose
    observations dropped (LmSize 1), Huber weights frozen at the start, cheirality not enforced on trial poses — fails
    the comparison of test_host_restatement_meets_numpy on its case, which the right LM passes."""
    s, o = _wrong_case(wrong)
    worst, same = _agree(hc, s, o)
    assert same and worst <= 1.0
    worst, same = _agree(hc, s, o, wrong=wrong)
    print(wrong, "worst ratio", worst, "statuses and counts agree", same)
    assert not same or worst > 1.0
