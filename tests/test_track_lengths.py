"""Track lengths at the edges of the linearisation ranges, checked without a GPU (cases: tests/track_cases.py).

1. expected_ranges, the Python restatement of the packing rule, on prefixes counted by hand.
2. ba_hostcheck_schur_lists on every case's graph with random Jacobians: the lists of structure.h reproduce the
   dense Schur complement (as tests/test_structure_lists.py, same 1e-11), the library's own range invariants hold
   (whole landmarks, every observation once, long tracks alone and last: return codes -2 .. -5), and the NUMBER of
   ranges is the one the packing rule gives — a rule that is off by one at 64 still covers every observation once.
3. The soundness gate: the oracle alone accepts every case (Solve(1) returns 0), every active pose has at least 9
   observations and cond(S) < 1e8 — 30 to 300 times over the cases as they stand (3e5 .. 3.4e6) — so an edit of the
   table cannot quietly make a case ill-posed and the tolerances of tests/test_track_lengths_gpu.py meaningless.
"""
import numpy as np
import pytest

import track_cases as tc
from helpers import brute_force_schur, fill, gn_options, hostcheck_lib, schur_lists

CASES = sorted(tc.cases(1))


@pytest.fixture(scope="module")
def hc():
    return hostcheck_lib()


def test_expected_ranges_on_hand_counted_prefixes():
    pre = tc.prefixes(1)
    assert tc.expected_ranges(pre["exact_64"]) == (3, 0)
    # 32+32 | 16+16+16+16 | 63+1 | 60+4 | 64 x 1
    assert tc.expected_ranges(pre["packed_to_64"]) == (5, 0)
    # LmSize 3 (2 for 1): 32+32 | 16+16+16+16 | 63 | 2+60 | 4 + 30 x 2 | 2 x 2
    assert tc.expected_ranges(tc.prefixes(3)["packed_to_64"]) == (6, 0)
    # 63 | 64 | (65) | 1 | 64 | (66): the 1 cannot join the 64 behind it
    assert tc.expected_ranges(pre["around_64"]) == (4, 2)
    assert tc.expected_ranges(pre["long_tracks"]) == (0, 6)
    assert tc.expected_ranges(pre["long_tracks_odd"]) == (0, 7)
    # 5 + 7 | (100) | 3: empty landmarks neither open nor close a range
    assert tc.expected_ranges(pre["empty_landmarks"]) == (2, 1)
    assert tc.expected_ranges([]) == (0, 0) and tc.expected_ranges([0, 0]) == (0, 0)
    assert tc.expected_ranges([64, 1]) == (2, 0) and tc.expected_ranges([1, 64]) == (2, 0)
    assert tc.expected_ranges([6] * 10) == (1, 0) and tc.expected_ranges([6] * 11) == (2, 0)
    for lm_dim in (1, 3):
        for name, lengths in tc.cases(lm_dim).items():
            n_small, n_big = tc.expected_ranges(lengths)
            assert n_big == len(tc.long_ids(lengths))
            assert (n_big > 0) == (name in tc.WITH_LONG), name


def _activity(rng, sc, lengths, lm):
    """some inactive poses and landmarks; an inactive long track and a long track whose reference pose is inactive"""
    pose_active = (rng.random(sc.num_poses) > 0.15).astype(np.uint8)
    lm_active = (rng.random(len(lengths)) > 0.1).astype(np.uint8)
    big = tc.long_ids(lengths)
    if len(big) >= 2:
        lm_active[big] = 1
        lm_active[big[0]] = 0
        lm_active[big[-1]] = 1
        pose_active[sc.lm_ref_pose[big[-1]]] = 0
    return pose_active, lm_active


# PoseSize 15 (blocks straddling the 64-row tiles) on half of the graphs: the dense reference is 2 O x 15 P
@pytest.mark.parametrize("name,LM,D", [(c, LM, 6) for c in CASES for LM in (1, 3)]
                         + [(c, LM, 15) for c in ("around_64", "exact_64", "long_tracks", "mixed") for LM in (1, 3)])
def test_lists_on_track_length_edges(hc, name, LM, D):
    lengths = tc.cases(LM)[name]
    sc, _, pp, pl = tc.build(LM, lengths)
    rng = np.random.default_rng(100 * LM + D + len(lengths))
    pose_active, lm_active = _activity(rng, sc, lengths, pl)
    lm_ref = np.ascontiguousarray(sc.lm_ref_pose, dtype=np.uint32)
    O = len(pp)
    jm, jr = rng.normal(size=(O, 12)), rng.normal(size=(O, 12))
    jl, r = rng.normal(size=(O, 2 * LM)), rng.normal(size=(O, 2))
    w = rng.uniform(0.3, 2.0, O)
    n = int(pose_active.sum()) * D
    S, S_lower, rhs_p, rhs_sc, counts = schur_lists(hc, LM, D, pose_active, lm_active, lm_ref, pp, pl, jm, jr, jl, r, w)
    S_ref, rhs_p_ref, rhs_sc_ref = brute_force_schur(LM, D, pose_active, lm_active, lm_ref, pp, pl, jm, jr, jl, r, w)
    assert np.abs(S - S_ref).max() < 1e-11 * np.abs(S_ref).max()
    assert np.abs(rhs_p[:n] - rhs_p_ref).max() < 1e-11 * max(np.abs(rhs_p_ref).max(), 1.0)
    assert np.abs(rhs_sc[:n] - rhs_sc_ref).max() < 1e-11 * max(np.abs(rhs_sc_ref).max(), 1.0)
    assert not S_lower[n:, :].any() and not S_lower[:, n:].any()
    n_small, n_big = tc.expected_ranges(lengths)
    assert counts[0] == n_small + n_big, (int(counts[0]), n_small, n_big)
    assert counts[7] == pose_active.sum()


@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_oracle_accepts_every_case(oracle_lib, name, lm_dim):
    po = oracle_lib
    lengths = tc.cases(lm_dim)[name]
    sc, z, pose, lm = tc.build(lm_dim, lengths)
    # residual ids are not sorted by landmark, and the table holds what it says
    assert (np.diff(lm.astype(np.int64)) < 0).any()
    assert np.array_equal(np.bincount(lm, minlength=len(lengths)), lengths)
    big = tc.long_ids(lengths)
    if len(big):   # drawn with replacement: a long track holds several observations from one pose
        assert len(np.unique(pose[lm == big[-1]])) < lengths[big[-1]]
    pa = tc.anchored(sc)
    o = po.OracleBundleAdjuster(lm_dim, 6)
    o.Init(gn_options(po, apply_results=0))
    fill(o, sc, active=pa)
    assert o.GetNumProjResiduals() == len(pose)
    o.Solve(1)
    cond = np.linalg.cond(tc.symmetric(o.S()))
    nobs = tc.observations_per_active_pose(sc, pose, lm, pa)
    print("%s LmSize %d: n_small %d n_big %d cond(S) %.3g min observations per pose %d"
          % ((name, lm_dim) + tc.expected_ranges(lengths) + (cond, nobs.min())))
    assert o.summary().result == 0
    assert nobs.min() >= 9
    assert cond < 1e8
