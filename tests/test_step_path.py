"""Soundness gate of the step-path checks (step_cases.py), on the CPU: the oracle's outputs and a plain float64
restatement of the step path stay inside every bound on every case, each of thirteen subtly wrong step paths fails
at least one bound on at least one case, and the cases have the block and partial counts they are built for.

The restatement takes the oracle's pose step: the reduced solve is not part of the step path (test_tile_factor*.py
own it), and a float64 LU of the same system misses the pose-row figure the oracle's L D L^T reaches by a factor of 6
to 13 on `edges_lm1` (measured: oracle 11 eps, LU of the full system 76 eps, LU of the Schur complement 140 eps), so
the bound of 8 x the oracle's figure is a bound on the back-substitution for a given pose step."""
import numpy as np
import pytest

import step_cases as sc
import track_cases as tc

CASES = sorted(sc.CASES)
_runs = {}


def _oracle(po, name):
    """one oracle run, its full-system figures and the restatement's bundle per case and process"""
    if name not in _runs:
        c = sc.case(name)
        o = sc.oracle_run(po, c)
        assert o.summary.result == 0
        (lm, _), (pose, _) = sc.system_ratios(c, o.lin, o.gn_p, o.gn_l)
        _runs[name] = (c, o, (lm, pose))
    return _runs[name]


def _restated(po, name, mutant=None):
    c, o, ratio = _oracle(po, name)
    return sc.restate(c, o.lin, o.gn_p, rhs_p=o.rhs_p if c.imu else None, mutant=mutant), ratio


@pytest.mark.parametrize("name", CASES)
def test_oracle_and_restatement_hold_every_bound(oracle_lib, name):
    c, o, ratio = _oracle(oracle_lib, name)
    # the oracle's vectors with the restatement's sums, steps and updates computed FROM them ...
    b, _ = _restated(oracle_lib, name)
    mixed = sc.types.SimpleNamespace(**vars(b))
    mixed.rhs_p, mixed.rhs_l, mixed.gn_l = o.rhs_p, o.rhs_l, o.gn_l
    figs_o = sc.compare(sc.types.SimpleNamespace(case=c, lin=o.lin, rhs_p=o.rhs_p, rhs_l=o.rhs_l, gn_p=o.gn_p, gn_l=o.gn_l), ratio)
    # ... and the restatement on its own
    figs = sc.compare(b, ratio)
    print("STEP %s: oracle landmark rows %.3g eps, pose rows %.3g eps; restatement %.3g, %.3g"
          % (name, ratio[0], ratio[1], figs["system.landmark_rows"].value,
             figs["system.pose_rows"].value if "system.pose_rows" in figs else np.nan))
    sc.report(name, figs)
    assert not sc.failures(figs_o) and not sc.failures(figs), (sc.failures(figs_o), sc.failures(figs))
    # conventions, independently of the Jacobians: the restated right-hand sides and landmark step are the oracle's
    assert np.abs(b.rhs_l - o.rhs_l).max() <= 1e-11 * np.abs(o.rhs_l).max()
    assert np.abs(b.rhs_p - o.rhs_p).max() <= 1e-11 * np.abs(o.rhs_p).max()
    assert np.linalg.norm(b.gn_l - o.gn_l) <= 1e-8 * np.linalg.norm(o.gn_l)
    assert len(figs) > 60


@pytest.mark.parametrize("name", CASES)
def test_float64_rotations_stay_under_four_eps(oracle_lib, name):
    """every rotation the ladder uses, both branches of so3_exp: the float64 restatement against long double"""
    b, _ = _restated(oracle_lib, name)
    worst, small, large = 0.0, 0, 0
    for i, u in enumerate(b.updates):
        f = {}
        sc.compare_update(f, "u", b.case, u)
        worst = max(worst, f["u.rotation"].value)
        th = np.linalg.norm(u.step_p[:b.case.n].reshape(-1, b.case.D)[:, 3:6], axis=1)
        small += int((th < sc.SMALL_ANGLE).sum())
        large += int((th > np.pi).sum())
    print("STEP %s: float64 rotations within %.3g eps of long double (%d under the small-angle threshold, %d beyond pi)"
          % (name, worst, small, large))
    assert worst <= sc.RESTATEMENT_ROTATION_BOUND and small > 0 and large > 0


# which case a wrong step path has to fail on (it may fail on more)
MUTANT_CASE = {
    "drop_block_last": "edges_lm1_last_active", "count_inactive_landmark": "edges_lm1",
    "jrhs_without_reference_pose": "edges_lm1", "jrhs_with_inactive_pose": "edges_lm3",
    "backsub_without_reference_row": "edges_lm1", "backsub_without_calibration": "tvs", "step_by_landmark_id": "edges_lm3",
    "left_multiply": "vi15", "sin_theta": "edges_lm1", "negative_kept": "edges_lm1", "revert_keeps_flag": "tvs",
    "tail_in_norm": "tvs", "zero_coefficient_reads_gn": "edges_lm3"}


@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_comparator_rejects_wrong_step_paths(oracle_lib, mutant):
    assert set(MUTANT_CASE) == set(sc.MUTANTS)
    b, ratio = _restated(oracle_lib, MUTANT_CASE[mutant], mutant)
    bad = sc.failures(sc.compare(b, ratio))
    print("STEP mutant %s on %s fails %d figures: %s" % (mutant, MUTANT_CASE[mutant], len(bad), ", ".join(bad[:6])))
    assert bad
    expect = {"drop_block_last": ("rhs_l_sq", "norm_l"), "count_inactive_landmark": ("rhs_l_sq",),
              "jrhs_without_reference_pose": ("j_rhs_sq",), "jrhs_with_inactive_pose": ("j_rhs_sq",),
              "backsub_without_reference_row": ("system.landmark_rows",), "backsub_without_calibration": ("system.landmark_rows",),
              "step_by_landmark_id": (".l",), "left_multiply": (".rotation",), "sin_theta": (".rotation",),
              "negative_kept": (".rho",), "revert_keeps_flag": (".flags",), "tail_in_norm": (".norm_p",),
              "zero_coefficient_reads_gn": ("_bitwise",)}[mutant]
    for part in expect:
        assert any(part in k for k in bad), (part, bad)


def test_case_invariants():
    for lm_dim in (1, 3):
        c = sc.case("edges_lm%d" % lm_dim)
        lopt, popt = sc.opt_ids(c.la), sc.opt_ids(c.pa)
        assert (c.P, int(c.pa.sum()), c.n) == (48, 44, 264) and -(-c.n // 256) == 2 and c.n - 256 == 8
        assert (c.L, c.O) == (257, 1285) and -(-c.O // 256) == 6 and c.O - 5 * 256 == 5
        assert -(-c.L // 256) == 2 and c.L - 256 == 1                       # landmark 256 alone in the second block
        assert not c.la[0] and not c.la[255] and bool(c.la[256]) == (lm_dim == 1)
        per_lm = np.bincount(c.lm, minlength=c.L)
        assert per_lm[c.no_residual] == 0 and c.la[c.no_residual] and per_lm[c.twice_seen] == 10
        if lm_dim == 1:     # seen from its reference pose only: the observation the residual list rejects
            seen = c.obs_pose[c.obs_lm == c.no_residual]
            assert list(seen) == [c.sc.lm_ref_pose[c.no_residual]]
        assert c.la[c.only_inactive] and not c.pa[c.pose[c.lm == c.only_inactive]].any()
        if lm_dim == 1:
            assert c.pa[c.sc.lm_ref_pose[c.only_inactive]]
            # inactive reference poses with active measuring poses and the other way round both occur
            assert (~c.pa[c.ref].astype(bool) & c.pa[c.pose].astype(bool)).any()
        assert c.masks[sc.REGULARISED_POSE] == 0x7 and c.pa[sc.REGULARISED_POSE] and np.count_nonzero(c.masks) == 1
        # ids by landmark and by optimisation index differ from landmark 1 on
        assert lopt[1] == 0 and lopt[256] == (254 if lm_dim == 1 else -1)
        assert len(np.unique(c.lm[:50])) > 40                               # residual ids are not sorted by landmark
    c = sc.case("edges_lm1_last_active")
    assert c.la[255] and not c.la[254] and c.O == 1285
    c = sc.case("vi15")
    assert (c.D, c.P, c.n, c.LM) == (15, 18, 270, 1) and c.pa.all() and -(-c.n // 256) == 2 and 60 <= c.L <= 80
    c = sc.case("tvs")
    assert (c.K, c.LM) == (6, 1) and 25 <= c.P <= 35 and 50 <= c.L <= 70
    counts = sc.chain_counts(sc.case("edges_lm3"), shards=2)
    assert max(counts.values()) < 64


def test_special_branches_are_taken(oracle_lib):
    """at least one landmark on each special branch, seen in the oracle's own numbers"""
    c, o, _ = _oracle(oracle_lib, "edges_lm1")
    H, g = sc.full_system(c, o.lin)
    lopt = sc.opt_ids(c.la)
    off = c.n + c.K
    i = off + lopt[c.no_residual]
    assert float(H[i, i]) == sc.V_GUARD and g[i] == 0 and o.gn_l[lopt[c.no_residual]] == 0.0     # the guard on V
    j = off + lopt[c.only_inactive]
    assert H[j, j] > 1 and np.count_nonzero(H[j, :c.n]) == 6        # coupled to its reference pose alone
    # a negative inverse depth: the rung built for it turns a known, non-empty subset negative
    b, _ = _restated(oracle_lib, "edges_lm1")
    w = sc.update_reference(c, b.updates[-1].before, b.updates[-1].step_p, b.updates[-1].step_l)
    assert 20 <= len(w.negative) <= 120 and (w.rel == 0).sum() == len(w.negative)
    assert (sc.update_reference(c, b.updates[3].before, b.updates[3].step_p, b.updates[3].step_l).rel == 1).all()
    # the calibration tail is large enough for the norm to notice it
    t, _ = _restated(oracle_lib, "tvs")
    s = t.steps[0]
    assert (s.step_p[t.case.n:] ** 2).sum() > 1e3 * sc.chain_counts(t.case)["norm_p"] * sc.EPS * (s.step_p[:t.case.n] ** 2).sum()


def test_error_sum_of_build_problem_and_partial_counts(oracle_lib):
    """BuildProblem's proj_error is the sum of w |r|^2 with the weights of that linearisation (the sum the `r` tap
    gives: it carries sqrt(w)); the long_sums cases sit on both sides of the 8192-partial threshold."""
    for name in ("edges_lm1", "edges_lm3", "tvs"):
        c, o, _ = _oracle(oracle_lib, name)
        tap = float((np.asarray(o.lin.r, dtype=sc.LD) ** 2).sum())
        assert abs(tap - o.summary.proj_error) <= 1e-13 * tap
        assert o.lin.w.min() < 1.0      # Huber weights are in play
    for L in (sc.L1_THRESHOLD, sc.L1_THRESHOLD + 1):
        c = sc.long_sums(L)
        per_lm = np.bincount(c.lm, minlength=L)
        assert (per_lm == sc.LONG_TRACK).all() and c.O == L * sc.LONG_TRACK
        assert tc.expected_ranges(per_lm) == (L, 0)
    assert sc.chain(sc.L1_THRESHOLD + 1) == 8 + (1 + 8) + (1 + 8) and sc.chain(sc.L1_THRESHOLD) == 8 + 32 + 8
