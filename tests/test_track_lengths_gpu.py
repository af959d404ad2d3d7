"""The projection path against the oracle where the track lengths sit on the edges of the linearisation ranges
(cases: tests/track_cases.py; their soundness without a GPU: tests/test_track_lengths.py).

k_linearize packs whole landmarks into wavefront ranges of at most 64 observations and runs a segmented scan over
the lanes of a range; a landmark with more than 64 observations gets a range of its own and the two-pass
instantiation of the kernel.  The other oracle-parity tests use scene.make_scene, where every landmark has the same
5 .. 10 observations.  Here: exactly 64, sums of exactly 64, 65 / 127 / 128 / 129 / 200 / 700 (a ragged last
pass), an odd number of long tracks, shards without a short track, empty landmarks next to long ones.

Tolerances of the single linearisation are those of test_reduced_system_and_step (tests/test_gpu_parity.py); every
test prints the figures it asserts ("TRACK ..." lines, pytest -s).  Every test asserts that the number of wavefront
ranges the engine built is the one track_cases.expected_ranges gives, and that the two-pass launch ran where the
case intends it.

Measured on an MI355X (worst over pinhole / FOV and robust norm on / off; relative errors against the oracle):

    case             LmSize  n_small n_big  cond(S)  Jacobians  S        rhs      weights  delta_p  delta_l
    exact_64           1       63      0    5.5e5    6.9e-15    6.7e-15  1.5e-14  1.1e-14  9.8e-14  4.4e-14
    exact_64           3       63      0    4.2e5    3.0e-15    7.0e-14  8.1e-14  3.7e-15  6.4e-12  2.0e-12
    packed_to_64       1       65      0    1.2e6    4.2e-15    2.4e-15  1.2e-14  5.2e-15  1.2e-13  1.5e-13
    packed_to_64       3       65      0    7.3e5    4.3e-15    5.4e-12  4.5e-12  5.9e-15  4.5e-10  7.3e-10
    around_64          1       64      2    1.2e6    6.5e-15    2.5e-15  1.0e-14  5.8e-15  2.1e-13  4.4e-14
    around_64          3       64      2    4.6e5    3.8e-15    2.5e-14  4.2e-14  4.7e-15  5.8e-12  2.2e-12
    long_tracks        1       60      6    3.2e6    8.0e-15    8.1e-15  2.0e-14  1.1e-14  4.4e-13  8.2e-14
    long_tracks        3       60      6    1.3e6    2.7e-15    1.3e-14  2.5e-14  3.3e-15  3.4e-12  1.2e-12
    long_tracks_odd    1       60      7    1.6e6    6.9e-15    4.8e-15  1.3e-14  7.5e-15  1.8e-13  4.6e-14
    long_tracks_odd    3       60      7    3.6e5    7.1e-15    1.8e-14  3.0e-14  9.8e-15  2.0e-12  8.7e-13
    only_long          1       61      4    1.9e6    6.2e-15    6.7e-15  1.3e-14  9.2e-15  2.4e-13  6.5e-14
    only_long          3       61      4    3.4e5    4.4e-15    3.4e-14  6.8e-14  3.8e-15  4.9e-12  1.4e-12
    empty_landmarks    1       61      1    4.2e6    1.2e-14    9.5e-15  1.5e-14  1.0e-14  2.3e-13  4.1e-14
    empty_landmarks    3       61      1    1.1e6    5.2e-15    2.0e-14  4.3e-14  7.4e-15  1.8e-11  2.4e-12
    mixed              1       74     12    4.1e6    9.8e-15    8.8e-15  4.7e-14  1.5e-14  1.9e-13  5.7e-14
    mixed              3       75     12    8.4e5    5.3e-15    6.0e-14  7.7e-14  7.9e-15  6.3e-12  1.4e-12

Iterations: final poses within 1.1e-13, landmarks within 5.6e-11; shards against one engine 3.2e-12; calibration
borders within 2.2e-14, delta_k 2.4e-13; landmark marginals within 6.5e-13.  The file takes 22 s.
"""
import threading

import numpy as np
import pytest

import track_cases as tc
from ba_amd import hipapi, scene, sharding
from helpers import rel_err
from test_gpu_parity import (T_VS_MOUNT, _calib_pair, _check_against_oracle, _intrinsics_pair, _oracle_gn_run,
                             _run_engine_steps, both)
from test_marginals_gpu import _blk_err, _engine, _landmark_reference, _solve, _tol

pytestmark = pytest.mark.gpu

CASES = sorted(tc.cases(1))


def _report(tag, **figs):
    print("TRACK %s %s" % (tag, " ".join("%s=%.3g" % kv for kv in figs.items())), flush=True)


def _assert_ranges(eng, lengths, name=None):
    """The engine's range count is the packing rule's.  structure_stats() has the total only; the split into small
    and two-pass ranges is held on the same graphs by the host builder's invariants (return code -4 of
    ba_hostcheck_schur_lists, tests/test_track_lengths.py) and carried to the device builder by
    test_kernel_variants_are_bitwise_identical (key 5: lists built on the host give bitwise the same S)."""
    n_small, n_big = tc.expected_ranges(lengths)
    assert eng.structure_stats()["linearize_waves"] == n_small + n_big
    if name in tc.WITH_LONG:
        assert n_big > 0
    return n_small, n_big


def _exact_S(o, sc, pose, lm, pa):
    """S of the oracle's per-residual Jacobians in numpy.longdouble (the algebra of helpers.brute_force_schur, summed
    landmark by landmark): the arbiter when an S misses its tolerance — measure the oracle's and the engine's S
    against it before touching a bound."""
    LM = sc.lm_dim
    ld = np.longdouble
    jm, jr, jl = (np.asarray(x, dtype=ld) for x in o.proj_jacobians())
    w = np.asarray(o.proj_weights(), dtype=ld)
    opt = np.full(sc.num_poses, -1)
    opt[pa > 0] = np.arange(int(pa.sum()))
    n = int(pa.sum()) * 6
    S = np.zeros((n, n), dtype=ld)
    for l in np.unique(lm):
        W, V = np.zeros((n, LM), dtype=ld), np.zeros((LM, LM), dtype=ld)
        ref = opt[sc.lm_ref_pose[l]]
        for a in np.nonzero(lm == l)[0]:
            J = np.zeros((2, n), dtype=ld)
            if opt[pose[a]] >= 0:
                J[:, 6 * opt[pose[a]]:6 * opt[pose[a]] + 6] += jm[a]
            if LM == 1 and ref >= 0:
                J[:, 6 * ref:6 * ref + 6] += jr[a]
            cols = np.nonzero(J.any(0))[0]
            S[np.ix_(cols, cols)] += w[a] * (J[:, cols].T @ J[:, cols])
            W += w[a] * (J.T @ jl[a])
            V += w[a] * (jl[a].T @ jl[a])
        Vi = np.array([[1 / V[0, 0]]], dtype=ld) if LM == 1 else np.asarray(np.linalg.inv(V.astype(np.float64)), dtype=ld)
        if LM == 3:   # two Newton steps take the float64 inverse to long double precision
            for _ in range(2):
                Vi = Vi @ (2 * np.eye(3, dtype=ld) - V @ Vi)
        rows = np.nonzero(W.any(1))[0]
        S[np.ix_(rows, rows)] -= W[rows] @ Vi @ W[rows].T
    return S


# ---- a. one linearisation -------------------------------------------------------------------------------------
# S is held to 1e-12 except where the oracle itself is further than that from the S formed in long double from its
# own Jacobians (_exact_S).  `packed_to_64` with LmSize 3 holds 33 landmarks seen from two poses only: their 3 x 3 V
# is poorly conditioned and W V^-1 W^T cancels digits on both sides.  Measured error of the ORACLE's S against the
# long-double S there: 2.67e-12 (pinhole, Huber), 2.19e-12 (pinhole, no robust norm), 2.06e-12 (FOV, Huber), 1.80e-12
# (FOV, no robust norm); every other case: 3e-16 .. 6e-14.  The engine's S against the same long-double S, measured
# on an MI355X in the same order: 1.27e-12, 1.04e-12, 4.62e-12, 4.05e-12 (engine against oracle: 3.3e-12 .. 5.4e-12) —
# both are off alike, with per-residual Jacobians that agree to 4e-15.  The bound of that case is 8 x the smallest of
# the oracle's four figures, and the engine's distance from the long-double S is held to the same bound.
S_TOLERANCE = {("packed_to_64", 3): 8 * 1.8e-12}


@pytest.mark.parametrize("robust", [1, 0], ids=["huber", "no_robust_norm"])
@pytest.mark.parametrize("camera", ["pinhole", "fov"])
@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_one_linearisation_matches_oracle(oracle_lib, name, lm_dim, camera, robust):
    """Per-residual Jacobians and residuals, weights, reduced system, right-hand sides, error and step of one
    linearisation (apply_results = 0) against the oracle.  Bound of S: see S_TOLERANCE above."""
    po = oracle_lib
    lengths = tc.cases(lm_dim)[name]
    sc, z, pose, lm = tc.build(lm_dim, lengths)
    if camera == "fov":
        scene.to_fov_camera(sc, 0.93)
    pa = tc.anchored(sc)
    o, h = both(po, sc, lm_dim, active=pa, apply_results=0, use_robust_norm_for_proj_residuals=robust)
    o.Solve(1)
    h.Solve(1)
    O = len(pose)
    assert o.GetNumProjResiduals() == h.GetNumProjResiduals() == O
    assert o.summary().result == h.summary().result == 0
    n_small, n_big = _assert_ranges(h.engine(), lengths, name)
    # the engine's blocks carry sqrt(w); pose blocks are compared where they enter the system (active poses)
    sw = np.sqrt(o.proj_weights())
    act_m, act_r = pa[pose][:, None, None], pa[sc.lm_ref_pose[lm]][:, None, None]
    jm_o, jr_o, jl_o = o.proj_jacobians()
    jm_o, jr_o, jl_o = jm_o * sw[:, None, None] * act_m, jr_o * sw[:, None, None] * act_r, jl_o * sw[:, None, None]
    r_o = o.proj_residuals() * sw[:, None]
    jm_h, jr_h, jl_h, r_h = h.engine().get_proj_jacobians(O)
    jm_h, jr_h = jm_h * act_m, jr_h * act_r
    big = np.isin(lm, tc.long_ids(lengths))
    figs = dict(
        n_small=n_small, n_big=n_big, cond=np.linalg.cond(tc.symmetric(o.S())),
        j_meas=rel_err(jm_h, jm_o), j_lm=rel_err(jl_h, jl_o), r=rel_err(r_h, r_o),
        j_ref=rel_err(jr_h, jr_o) if lm_dim == 1 else 0.0,
        j_long=rel_err(jm_h[big], jm_o[big]) if big.any() else 0.0,
        S=rel_err(h.S(), o.S()), rhs=rel_err(h.rhs(), o.rhs()), rhs_p=rel_err(h.rhs_p(), o.rhs_p()),
        rhs_l=rel_err(h.rhs_l(), o.rhs_l()), w=rel_err(h.proj_weights(), o.proj_weights()),
        err=abs(h.summary().proj_error - o.summary().proj_error) / o.summary().proj_error,
        dp=rel_err(h.delta_p(), o.delta_p()), dl=rel_err(h.delta_l(), o.delta_l()))
    _report("a %s lm%d %s robust%d" % (name, lm_dim, camera, robust), **figs)
    s_tol = S_TOLERANCE.get((name, lm_dim), 1e-12)
    if not figs["S"] < 1e-12:   # arbitration figures, before anything fails (S is kept in the upper triangle)
        Sx = np.triu(_exact_S(o, sc, pose, lm, pa))
        arb = dict(oracle=rel_err(np.triu(o.S()).astype(np.longdouble), Sx),
                   engine=rel_err(np.triu(h.S()).astype(np.longdouble), Sx))
        _report("a-arbiter %s lm%d %s robust%d" % (name, lm_dim, camera, robust), **arb)
        if s_tol > 1e-12:      # a widened case: the engine is no further from the exact S than the bound allows either
            assert arb["engine"] < s_tol
    for k in ("j_meas", "j_ref", "j_lm", "r", "j_long"):
        assert figs[k] < 1e-11, k
    if lm_dim == 1:
        assert np.abs(jr_o).max() > 0
    assert figs["S"] < s_tol
    assert figs["rhs"] < 1e-11 and figs["rhs_p"] < 1e-11 and figs["rhs_l"] < 1e-11
    assert figs["w"] < 1e-12
    if robust:
        assert o.proj_weights().min() < 1.0
    assert figs["err"] < 1e-10
    assert figs["dp"] < 1e-8 and figs["dl"] < 1e-8


# ---- b. iterations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dogleg", [0, 1], ids=["gauss_newton", "dogleg"])
@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("name", ["long_tracks", "mixed"])
def test_iterations_track_oracle(oracle_lib, name, lm_dim, dogleg):
    """Four Solve(1) steps (Gauss-Newton; dogleg with trust_region_size 0.05) with the bars of
    test_gauss_newton_iterations_track_oracle / test_dogleg_matches_oracle; reliability flags and outlier ratios of
    every landmark are equal.  `long_tracks` with LmSize 1 carries 2 % gross mismatches, in the added observations
    too: Huber weights and outlier counts are not trivial on the long tracks.  Not with LmSize 3: there the oracle
    alone sends a six-view landmark with a mismatch to 2e6 m by the third iteration, cond(V) 5e8 .. 3e14 (the 3-D
    parametrisation has no guard like the inverse-depth one), and that one landmark decides the norm of the state."""
    po = oracle_lib
    lengths = tc.cases(lm_dim)[name]
    sc, z, pose, lm = tc.build(lm_dim, lengths, outlier_frac=0.02 if (name, lm_dim) == ("long_tracks", 1) else 0.0)
    pa = tc.anchored(sc)
    kw = dict(use_dogleg=1, trust_region_size=0.05) if dogleg else {}
    o, h = both(po, sc, lm_dim, active=pa, **kw)
    worst = dict(proj_error=0.0, delta_norm=0.0, trust=0.0, pre=0.0, post=0.0)
    for it in range(4):
        o.Solve(1)
        h.Solve(1)
        so, sh = o.summary(), h.summary()
        assert so.result == sh.result
        if dogleg:
            worst["trust"] = max(worst["trust"], abs(so.trust_region_size - sh.trust_region_size) / max(abs(so.trust_region_size), 1e-300))
            worst["pre"] = max(worst["pre"], abs(so.pre_solve_norm - sh.pre_solve_norm) / so.pre_solve_norm)
            worst["post"] = max(worst["post"], abs(so.post_solve_norm - sh.post_solve_norm) / so.post_solve_norm)
            worst["delta_norm"] = max(worst["delta_norm"], abs(so.delta_norm - sh.delta_norm) / max(so.delta_norm, 1e-12))
            assert abs(so.trust_region_size - sh.trust_region_size) <= 1e-7 * abs(so.trust_region_size)
            assert abs(so.pre_solve_norm - sh.pre_solve_norm) < 1e-8 * so.pre_solve_norm
            assert abs(so.post_solve_norm - sh.post_solve_norm) < 1e-8 * so.post_solve_norm
            assert abs(so.delta_norm - sh.delta_norm) < 1e-6 * max(so.delta_norm, 1e-12)
        else:
            worst["proj_error"] = max(worst["proj_error"], abs(so.proj_error - sh.proj_error) / so.proj_error)
            worst["delta_norm"] = max(worst["delta_norm"], abs(so.delta_norm - sh.delta_norm) / so.delta_norm)
            assert abs(so.proj_error - sh.proj_error) < 1e-8 * so.proj_error
            assert abs(so.delta_norm - sh.delta_norm) < 1e-7 * so.delta_norm
    _assert_ranges(h.engine(), lengths, name)
    poses_err, lms_err = rel_err(h.poses()[0], o.poses()[0]), rel_err(h.landmarks(), o.landmarks())
    _report("b %s lm%d dogleg%d" % (name, lm_dim, dogleg), poses=poses_err, landmarks=lms_err, **worst)
    assert poses_err < 1e-8
    assert lms_err < 1e-8
    rel_o = np.array([o.IsLandmarkReliable(l) for l in range(len(lengths))])
    rel_h = np.array([h.IsLandmarkReliable(l) for l in range(len(lengths))])
    out_o = np.array([o.LandmarkOutlierRatio(l) for l in range(len(lengths))])
    out_h = np.array([h.LandmarkOutlierRatio(l) for l in range(len(lengths))])
    assert np.array_equal(rel_o, rel_h)
    assert np.array_equal(out_o, out_h)
    assert out_o[tc.long_ids(lengths)].max() > 0


# ---- c. shards: one of them without a single short track --------------------------------------------------------
def _shard_engine(sc, lm_dim, pa, z, pose, lm, ids):
    ids = np.asarray(ids)
    new_id = np.full(sc.num_landmarks, -1, dtype=np.int64)
    new_id[ids] = np.arange(len(ids))
    sel = new_id[lm] >= 0
    eng = hipapi.Engine(lm_dim, 6)
    eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks[ids], sc.lm_ref_pose[ids])
    eng.set_projection_residuals(z[sel], pose[sel], new_id[lm[sel]].astype(np.uint32))
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
    return eng


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_shard_of_long_tracks_only(oracle_lib, lm_dim):
    """`mixed` on two engines with the in-process all-reduce: shard 0 holds exactly the long tracks (no small range:
    the first launch of k_linearize is skipped there), shard 1 everything else.  Three iterations against one
    engine at 1e-9 and against the oracle."""
    lengths = np.asarray(tc.cases(lm_dim)["mixed"])
    sc, z, pose, lm = tc.build(lm_dim, lengths)
    pa = tc.anchored(sc)
    L = len(lengths)
    long_, rest = tc.long_ids(lengths), np.nonzero(lengths <= 64)[0]
    single = _shard_engine(sc, lm_dim, pa, z, pose, lm, np.arange(L))
    _assert_ranges(single, lengths, "mixed")
    out = {}
    _run_engine_steps(single, 3, out, "single")
    parts = [long_, rest]
    engs = [_shard_engine(sc, lm_dim, pa, z, pose, lm, ids) for ids in parts]
    assert _assert_ranges(engs[0], lengths[long_]) == (0, len(long_))
    assert _assert_ranges(engs[1], lengths[rest])[1] == 0
    ar = sharding.ThreadAllReduce(2)
    for r in range(2):
        engs[r].set_allreduce(ar.hook(r), r, 2)
    th = [threading.Thread(target=_run_engine_steps, args=(engs[r], 3, out, r)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not ar.failed
    for k in ("single", 0, 1):
        assert not isinstance(out[k], Exception), out[k]
    worst = 0.0
    for it in range(3):
        a, b0, b1 = out["single"][it], out[0][it], out[1][it]
        assert b0 == b1 or np.allclose(b0, b1, rtol=1e-12)
        assert a[0] == b0[0] == 0
        for x, y in zip(a[1:], b0[1:]):
            worst = max(worst, abs(x - y) / max(abs(x), 1e-12))
            assert abs(x - y) <= 1e-9 * max(abs(x), 1e-12)
    ps, _, _ = single.get_poses(sc.num_poses)
    p0, _, _ = engs[0].get_poses(sc.num_poses)
    p1, _, _ = engs[1].get_poses(sc.num_poses)
    _report("c mixed lm%d" % lm_dim, sums=worst, poses=rel_err(p0, ps))
    assert rel_err(p0, ps) < 1e-9 and np.array_equal(p0, p1)
    ref = _oracle_gn_run(oracle_lib, sc, lm_dim, pa, 3)
    _check_against_oracle(ref, out, "single", ps)
    _check_against_oracle(ref, out, 0, p0)
    for e_ in engs + [single]:
        e_.end_solve()
    lms = np.empty((L, 4))
    for r in range(2):
        lms[parts[r]] = engs[r].get_landmarks(len(parts[r]))
    assert rel_err(lms, ref[3]) < 1e-8
    assert rel_err(lms, single.get_landmarks(L)) < 1e-9
    for e_ in engs + [single]:
        e_.close()


# ---- d. calibration: the two-pass kernel of the calibration instantiations, with real measurements ---------------
def _calibration_scene():
    """`long_tracks` (LmSize 1) on the banked trajectory of the calibration tests, every third vehicle pose held
    at ground truth, as _calib_scene / _intrinsics_scene of tests/test_gpu_parity.py."""
    lengths = tc.cases(1)["long_tracks"]
    sc, z, pose, lm = tc.build(1, lengths, roll_amp=0.6)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[::3] = 0
    return lengths, sc, pa


def _bordered_figures(o, h, K):
    n = o.num_pose_params()
    assert h.num_pose_params() == n and h.engine().num_calib_params() == K
    So, Sh = o.S(), h.S()
    assert Sh.shape == (n + K, n + K)
    return dict(S_pp=rel_err(Sh[:n, :n], So[:n, :n]), S_pk=rel_err(Sh[:n, n:], So[:n, n:]),
                S_kk=rel_err(Sh[n:, n:], So[n:, n:]), rhs=rel_err(h.rhs(), o.rhs()), rhs_k=rel_err(h.rhs_k(), o.rhs_k()),
                dp=rel_err(h.delta_p(), o.delta_p()), dk=rel_err(h.delta_k(), o.delta_k()),
                dl=rel_err(h.delta_l(), o.delta_l()), cond=np.linalg.cond(tc.symmetric(So)))


def _assert_bordered(figs):
    """the bars of test_calibration_reduced_system_and_step"""
    assert figs["j_k"] < 1e-11
    assert figs["S_pp"] < 1e-12
    assert figs["S_pk"] < 1e-11 and figs["S_kk"] < 1e-11
    assert figs["rhs"] < 1e-11 and figs["rhs_k"] < 1e-11
    assert figs["dp"] < 1e-8 and figs["dk"] < 1e-8 and figs["dl"] < 1e-8


def test_mount_calibration_on_long_tracks(oracle_lib):
    """do_tvs: dz_dtvs per residual, S with its border, rhs, rhs_k and the step [delta_p ; delta_k], delta_l."""
    po = oracle_lib
    lengths, sc, pa = _calibration_scene()
    scene.mount_camera(sc, T_VS_MOUNT)
    sc.poses[::3] = sc.gt_poses[::3]
    t0 = po.exp_decoupled(T_VS_MOUNT, np.array([0.06, -0.05, 0.05, 0.02, -0.03, 0.02]))
    sc.landmarks = scene.remount_landmarks(sc, T_VS_MOUNT, t0)
    o, h = _calib_pair(po, sc, pa, t0, apply_results=0)
    o.Solve(1)
    h.Solve(1)
    assert o.summary().result == h.summary().result == 0
    assert _assert_ranges(h.engine(), lengths, "long_tracks")[1] == 6
    w = np.sqrt(o.proj_weights())[:, None, None]
    figs = _bordered_figures(o, h, 6)
    figs["j_k"] = rel_err(h.proj_tvs_jacobians(), w * o.proj_tvs_jacobians())
    _report("d long_tracks tvs", **figs)
    assert np.abs(o.S()[:o.num_pose_params(), o.num_pose_params():]).max() > 1
    _assert_bordered(figs)


def test_intrinsics_calibration_on_long_tracks(oracle_lib):
    """calib_size 4: dz_dcam_params per residual, the bordered system and the step."""
    po = oracle_lib
    lengths, sc, pa = _calibration_scene()
    sc.poses[::3] = sc.gt_poses[::3]
    wrong = np.asarray(sc.cam_params) * np.array([1.03, 0.97, 1.02, 0.98])
    o, h = _intrinsics_pair(po, sc, pa, wrong, apply_results=0)
    o.Solve(1)
    h.Solve(1)
    assert o.summary().result == h.summary().result == 0
    assert _assert_ranges(h.engine(), lengths, "long_tracks")[1] == 6
    w = np.sqrt(o.proj_weights())[:, None, None]
    figs = _bordered_figures(o, h, 4)
    figs["j_k"] = rel_err(h.proj_calib_jacobians(), w * o.proj_calib_jacobians())
    _report("d long_tracks intrinsics", **figs)
    assert np.abs(o.S()[:o.num_pose_params(), o.num_pose_params():]).max() > 0.1
    _assert_bordered(figs)


# ---- e. landmark marginals -------------------------------------------------------------------------------------
def _bare_landmark_reference(S, lm_dim):
    """(l, l) block of inv(H) for a landmark without observations: W = 0 and V = 0, which the guard of
    BundleAdjuster.cpp:431-439 (as restated in helpers.brute_force_schur) changes before the inversion."""
    n = S.shape[0]
    V = np.zeros((lm_dim, lm_dim))
    if lm_dim == 1:
        if abs(V[0, 0]) < 1e-6:
            V[0, 0] += 1e-6
    elif np.linalg.norm(V) < 1e-6:
        V += 1e-6 * np.eye(3)
    H = np.block([[S, np.zeros((n, lm_dim))], [np.zeros((lm_dim, n)), V]])
    return np.linalg.inv(H)[n:, n:]


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_landmark_marginals_on_track_length_edges(lm_dim):
    """landmark_marginals on `mixed` for every long track, two landmarks of exactly 64 observations, a landmark with
    one (LmSize 3: two) observations and an empty one, against inv(H) as tests/test_marginals_gpu.py forms it (the
    Jacobians it is formed from are checked against the oracle above); unary priors and odometry keep cond(S) in
    that file's range.  A landmark without observations is in no linearisation range; its block comes from the dense
    inverse of H with W = 0 and the guarded V (_bare_landmark_reference).  The engine returned zeros there (V^-1 is
    never written for such a landmark) until k_selinv.hip applied the guard.  ids=None equals the per-id calls bit
    for bit."""
    lengths = np.asarray(tc.cases(lm_dim)["mixed"])
    sc, z, pose, lm = tc.build(lm_dim, lengths)
    pa = tc.anchored(sc)
    pa[::9] = 0
    s = _engine(sc, lm_dim, pa, pose_pose=True, obs=(z, pose, lm))
    _assert_ranges(s.eng, lengths, "mixed")
    _solve(s)
    S = s.eng.get_S()
    tol = _tol(S)
    short = 1 if lm_dim == 1 else 2
    ids = list(tc.long_ids(lengths)) + list(np.nonzero(lengths == 64)[0][:2]) + [int(np.nonzero(lengths == short)[0][0])]
    assert len(ids) == 12 + 2 + 1
    got = s.eng.landmark_marginals(ids)
    want = _landmark_reference(s, S, [int(l) for l in ids])
    errs = [_blk_err(got[q], want[q]) for q in range(len(ids))]
    _report("e mixed lm%d" % lm_dim, worst=max(errs), tol=tol, cond=np.linalg.cond(S))
    for q in range(len(ids)):
        assert errs[q] <= tol, (ids[q], lengths[ids[q]])
    empty = np.nonzero(lengths == 0)[0]
    assert len(empty) >= 4
    bare = s.eng.landmark_marginals(empty)
    want_bare = _bare_landmark_reference(S, lm_dim)
    assert np.abs(want_bare).max() > 1e5
    for q in range(len(empty)):
        assert _blk_err(bare[q], want_bare) <= tol, empty[q]
    every = s.eng.landmark_marginals(None)
    per = s.eng.landmark_marginals(np.arange(len(lengths)))
    assert np.array_equal(every, per)
    s.eng.close()


# ---- f. kernel variants behind ba_hip_debug_set ---------------------------------------------------------------------
def _variant_run(sc, lm_dim, pa, z, pose, lm, keys):
    eng = hipapi.Engine(lm_dim, 6)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 1
    o.use_triangular_matrices = 1
    o.keep_reduced_system = 1
    eng.set_options(o)
    for k, v in keys.items():
        eng.debug_set(k, v)
    eng.set_cameras(sc.cam_params, [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose)
    eng.set_projection_residuals(z, pose, lm)
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(np.zeros(sc.num_poses, dtype=np.uint16))
    eng.linearize()
    S, rhs, w = eng.get_S(), eng.get_rhs(), eng.get_proj_weights(len(pose))
    waves = eng.structure_stats()["linearize_waves"]
    eng.end_solve()
    eng.close()
    return S, rhs, w, waves


@pytest.mark.parametrize("lm_dim", [1, 3])
def test_kernel_variants_are_bitwise_identical(lm_dim):
    """include/ba_hip.h ships the keys of ba_hip_debug_set as "kernel variants with identical results"; DESIGN.md
    section 4b: "kernel variants selectable at run time through ba_hip_debug_set, all bitwise identical"; k_reduce.hip
    on variant 6: "Bitwise the S of VAR 5".  Held here on `mixed`: key 4 (direct-store linearisation), key 1 (tile
    assembly variants 0, 1, 2, 6 against 5), key 2 (tile order) and key 3 (all tiles) give bitwise the same S —
    key 4 also the same right-hand sides and weights; so do the static lists built on the host (key 5), whose split
    into small and two-pass ranges tests/test_track_lengths.py checks on this graph.  The assembly variants 3 and 4
    were timing floors that left S wrong by design; they are no longer in the library and the key refuses them."""
    lengths = tc.cases(lm_dim)["mixed"]
    sc, z, pose, lm = tc.build(lm_dim, lengths)
    pa = tc.anchored(sc)
    n_small, n_big = tc.expected_ranges(lengths)
    S0, rhs0, w0, waves = _variant_run(sc, lm_dim, pa, z, pose, lm, {})
    assert waves == n_small + n_big and n_big > 0
    assert np.abs(S0).max() > 0 and np.isfinite(S0).all()
    S5, _, _, _ = _variant_run(sc, lm_dim, pa, z, pose, lm, {1: 5, 2: 0, 3: 0, 4: 0})
    assert np.array_equal(S5, S0), "the defaults are variant 5, row-major tiles, the factor's pattern, staged rows"
    S, rhs, w, _ = _variant_run(sc, lm_dim, pa, z, pose, lm, {4: 1})
    assert np.array_equal(S, S0) and np.array_equal(w, w0)
    for a, b in zip(rhs, rhs0):
        assert np.array_equal(a, b)
    for var in (0, 1, 2, 6):
        S, _, _, _ = _variant_run(sc, lm_dim, pa, z, pose, lm, {1: var})
        assert np.array_equal(S, S0), var
    for key in (2, 3):
        S, _, _, _ = _variant_run(sc, lm_dim, pa, z, pose, lm, {key: 1})
        assert np.array_equal(S, S0), key
    S, rhs, w, waves_host = _variant_run(sc, lm_dim, pa, z, pose, lm, {5: 1})
    assert waves_host == waves and np.array_equal(S, S0) and np.array_equal(w, w0)
    for a, b in zip(rhs, rhs0):
        assert np.array_equal(a, b)
    eng = hipapi.Engine(lm_dim, 6)
    for var in (3, 4, 7, -1):
        with pytest.raises(hipapi.HipError):
            eng.debug_set(1, var)
    eng.close()
