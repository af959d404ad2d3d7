"""Static structure of ba_hip_finalize (ba_amd/csrc/structure.h), checked on the CPU.

`ba_hostcheck_schur_lists` builds the lists for a random graph and evaluates them exactly as the
device kernels do (observation-major factor rows, tile references of the off-diagonal blocks,
per-pose terms of the diagonal blocks and right-hand sides).  Here the result is compared with a
dense brute-force restatement of the reference's algebra from the same per-residual Jacobians:
    U = J_p^T J_p,  W = J_p^T J_l,  V = J_l^T J_l (+ guard),  S = U - W V^-1 W^T,
    rhs_p = J_p^T r,  rhs_sc = rhs_p - W V^-1 J_l^T r
(/root/reference/src/BundleAdjuster.cpp:327-485).  Index logic only — the Jacobians are random.
Covers: inactive poses and landmarks, unlisted observations (measured from the reference pose),
duplicate observations of a landmark from one pose, landmarks with more than 64 observations,
landmarks without observations, PoseSize 6 / 9 / 15 (blocks straddling 64-tile boundaries).
Track lengths here are drawn from 0..kmax (kmax <= 12) plus one fixed 150; the edges of the range packing (exactly
64, sums of 64, 65 / 128 / 129, empty landmarks next to long tracks) and the range COUNT are the subject of
tests/test_track_lengths.py, on the graphs of tests/track_cases.py and with the helpers shared through helpers.py.
"""
import numpy as np
import pytest

from helpers import brute_force_schur, hostcheck_lib, schur_lists

@pytest.fixture(scope="module")
def hc():
    return hostcheck_lib()


def _random_graph(rng, P, L, LM, kmax, big=False):
    pose_active = (rng.random(P) > 0.15).astype(np.uint8)
    lm_active = (rng.random(L) > 0.1).astype(np.uint8)
    lm_ref = rng.integers(0, P, L).astype(np.uint32)
    pp, pl = [], []
    for l in range(L):
        k = int(rng.integers(0, kmax + 1))
        if LM == 3 and k == 1:
            k = 2                        # one view leaves the 3x3 V singular (inf on both sides)
        if big and l == L // 2:
            k = 150                      # more than one wave of observations
        poses = rng.integers(0, P, k)
        if k >= 3 and rng.random() < 0.3:
            poses[1] = poses[0]          # duplicate observation from one pose
        if k >= 2 and rng.random() < 0.3:
            poses[-1] = lm_ref[l]        # measured from the reference pose (second camera): unlisted for LM 1
        pp += list(poses)
        pl += [l] * k
    perm = rng.permutation(len(pp))      # residual ids are NOT sorted by landmark
    return pose_active, lm_active, lm_ref, np.array(pp, dtype=np.uint32)[perm], np.array(pl, dtype=np.uint32)[perm]


@pytest.mark.parametrize("LM,D,P,L,kmax,big", [(1, 6, 40, 60, 8, False), (3, 6, 40, 60, 8, False),
                                                (1, 15, 30, 50, 6, True), (3, 9, 25, 40, 6, True),
                                                (1, 6, 5, 8, 3, False), (1, 6, 120, 300, 12, True)])
def test_lists_reproduce_the_dense_schur_complement(hc, LM, D, P, L, kmax, big):
    rng = np.random.default_rng(1000 * LM + D + P)
    pose_active, lm_active, lm_ref, pp, pl = _random_graph(rng, P, L, LM, kmax, big)
    O = len(pp)
    jm, jr = rng.normal(size=(O, 12)), rng.normal(size=(O, 12))
    jl, r = rng.normal(size=(O, 2 * LM)), rng.normal(size=(O, 2))
    w = rng.uniform(0.3, 2.0, O)
    n = int(pose_active.sum()) * D
    S, S_lower, rhs_p, rhs_sc, counts = schur_lists(hc, LM, D, pose_active, lm_active, lm_ref, pp, pl, jm, jr, jl, r, w)
    S_ref, rhs_p_ref, rhs_sc_ref = brute_force_schur(LM, D, pose_active, lm_active, lm_ref, pp, pl, jm, jr, jl, r, w)
    scale = np.abs(S_ref).max()
    assert np.abs(S - S_ref).max() < 1e-11 * scale
    assert np.abs(rhs_p[:n] - rhs_p_ref).max() < 1e-11 * max(np.abs(rhs_p_ref).max(), 1.0)
    assert np.abs(rhs_sc[:n] - rhs_sc_ref).max() < 1e-11 * max(np.abs(rhs_sc_ref).max(), 1.0)
    # nothing outside the n x n system, nothing above the diagonal tiles
    assert not S_lower[n:, :].any() and not S_lower[:, n:].any()
    assert counts[0] >= 1 and counts[7] == pose_active.sum()
