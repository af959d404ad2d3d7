"""The reference of the per-block tests of the pose-pose assembly, checked on the CPU (posepose_cases.py; the device
side is test_pose_pose_blocks_gpu.py):

1. the oracle's own S equals the numpy sum of J^T Lambda J over its Jacobian taps, per block, to 1e-12;
2. the comparator block_errors rejects seven subtly wrong assemblies at the tolerance the device is held to, one
   of which the whole-matrix norm of the older tests accepts;
3. the host build of the inertial kernels' math against the oracle for every sample count of the imu_samples case;
4. the numpy dogleg denominator reproduces the oracle's dogleg step, and the graph is well enough conditioned for
   the solve check."""
import ctypes

import numpy as np
import pytest

from helpers import hostcheck_lib, rel_err
import leverage_cases as lc
import posepose_cases as pp
from pplever_cases import informations

CASES = {"graph6": pp.graph6, "imu_samples_15": lambda: pp.imu_samples(15), "imu_samples_9": lambda: pp.imu_samples(9)}


def _ref(po, name):
    return pp.cached_reference(po, name, CASES[name])


# ---- 1. soundness of the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_system_is_the_sum_of_its_residual_blocks(oracle_lib, name):
    """S of the oracle against triu(J^T J) of the whitened rows built from its taps, and against the same sum taken
    block by block (what the mutations below start from); every block relative to its own scale."""
    ref = _ref(oracle_lib, name)
    c = ref.case
    err = pp.block_errors(ref.S_oracle, ref.S, ref.scale, c.D, ref.undefined_blocks)
    own = pp.block_errors(pp.assemble(ref.blocks, c.D, c.pa, ref.masks), ref.S, ref.scale, c.D)
    print("%s: oracle S against the numpy sum %.3g at block %s; block-wise sum against J^T J %.3g; %d blocks undefined"
          % (name, err.worst, err.where, own.worst, len(ref.undefined_blocks)))
    assert pp.accepted(err, 1e-12) and pp.accepted(own, 1e-12)
    absent = int((ref.scale[np.triu_indices_from(ref.scale)] == 0).sum())
    assert absent > 0, "no absent pair in the case"


def test_graph6_is_the_graph_it_claims_to_be(oracle_lib):
    ref = _ref(oracle_lib, "graph6")
    c, t = ref.case, ref.case.t
    assert t.counts == (67, 101, 0) and int(c.pa.sum()) == 66
    down = int((ref.un_scale < 1.0).sum())
    print("graph6: the Huber pass down-weights %d of 67 priors" % down)
    assert 0.05 * 67 <= down <= 0.5 * 67, "the case does not test the Huber pass"
    # the two error sums of the reference: one formula for the unary kind, two for the binary (quirk Q5)
    assert abs(ref.built_unary_error - ref.unary_error) <= 1e-12 * ref.unary_error
    assert ref.built_binary_error > 10 * ref.binary_error > 0
    pairs = list(zip(t.bin_p1.tolist(), t.bin_p2.tolist()))
    assert sum(a > b for a, b in pairs) >= 13 and len(set(pairs)) < len(pairs)
    assert max(np.bincount(np.concatenate([t.bin_p1, t.bin_p2]))) >= 16      # the hub
    assert np.bincount(t.un_pose)[3] == 4 and np.bincount(t.un_pose)[30] == 2 and not c.pa[30]
    # the far loop closures are alone in their 64 x 64 tiles
    opt = pp.natural_rows(c.pa, 6)
    assert opt[40] // 64 - opt[7] // 64 >= 2 and opt[69] // 64 - opt[0] // 64 >= 2


def test_second_solve_compounds_the_unary_scales(oracle_lib):
    """quirk Q4: the oracle multiplies each Huber weight into cov_inv, so a second Solve(1) at the same state sees
    distances already scaled.  compounded_scales reproduces its second S."""
    ref = _ref(oracle_lib, "graph6")
    twice = pp.cached_reference(oracle_lib, "graph6 twice", pp.graph6, solves=2)
    err = pp.block_errors(twice.S_oracle, twice.S, twice.scale, 6)
    moved = np.abs(twice.un_scale - ref.un_scale).max()
    print("graph6, second Solve(1): oracle S against the numpy sum %.3g; the scales moved by up to %.3g" % (err.worst, moved))
    assert pp.accepted(err, 1e-12) and moved > 1e-3
    assert abs(twice.unary_error - ref.unary_error) > 1e-3 * ref.unary_error


def test_masks_applied_in_numpy_equal_the_oracles_own(oracle_lib):
    """The oracle masks the translation of pose 2 itself (RegularizePose) in one run and not in the other, where
    apply_masks does it: the same S and gradient, bit for bit.  (Its rotation flag cannot express 0x38.)"""
    c = pp.graph6()
    m = np.zeros(len(c.pa), np.uint16)
    m[2] = 0x7
    native = pp.reference(oracle_lib, c, masks=m, regularize=(2,))
    ours = pp.reference(oracle_lib, c, masks=m)
    assert np.array_equal(native.S_oracle, ours.S_oracle) and np.array_equal(native.rhs_oracle, ours.rhs_oracle)
    rows = pp.natural_rows(c.pa, 6)[2]
    assert np.all(np.diag(native.S_oracle)[rows:rows + 3] == pp.MASK_DIAGONAL)


def test_two_sample_information_is_undefined_in_the_oracle_too(oracle_lib):
    """why reference() leaves the blocks of the 2-sample residuals out: their information is not even symmetric"""
    ref = _ref(oracle_lib, "imu_samples_15")
    assert len(ref.undefined) == 12
    for i in range(ref.case.t.counts[2]):
        m = ref.imu_cov_inv_oracle[i]
        asym = np.abs(m - m.T).max() / np.abs(m).max()
        assert (asym > 1e-6 and np.abs(m).max() > 1e15) if i in ref.undefined else asym < 1e-12, (i, asym)


# ---- 2. the comparator ----------------------------------------------------------------------------------------
def _mutated(ref, kind):
    c, t, D = ref.case, ref.terms, 6
    nu = t.counts[0]
    blocks, masks = ref.blocks, ref.masks
    kw = {}
    if kind == "reversed_pair_not_transposed":
        kw["untransposed"] = {nu + c.reversed_pair}
    elif kind == "second_duplicate_dropped":
        kw["skip"] = {nu + c.dup_second}
    elif kind == "weak_block_dropped":
        kw["skip"] = {nu + c.weak}
    elif kind == "inactive_side_added":
        # (5, 30) itself has no active end; (12, 30) is the nearest edge with one: the block of its inactive
        # pose 30 lands on the diagonal of pose 12
        q = nu + c.half_active
        assert (t.p1[q], t.p2[q]) == (12, 30)
        j2 = ref.dz[q, 1, :6, :6]
        kw["extra"] = [(12, 12, j2.T @ ref.lam[q, :6, :6] @ j2)]
    elif kind == "masked_column_not_skipped":
        loose = masks.copy()
        loose[2] = 0x3
        blocks = pp.residual_blocks(t, D, ref.dz, ref.lam, c.pa, loose)
    elif kind == "median_one_too_low":
        md = np.einsum("ni,nij,nj->n", ref.raw_unary, ref.un_info, ref.raw_unary)
        info, w = informations(t, un_scale=pp.huber_scales(md, shift=-1))
        blocks = pp.residual_blocks(t, D, ref.dz, info * w[:, None, None], c.pa, masks)
    elif kind == "no_rotation_rule_omitted":
        info, w = informations(c.t, un_scale=ref.un_scale)     # (c.t: the information as handed over)
        blocks = pp.residual_blocks(t, D, ref.dz, info * w[:, None, None], c.pa, masks)
    else:
        raise KeyError(kind)
    return pp.assemble(blocks, D, c.pa, masks, **kw)


MUTATIONS = ["reversed_pair_not_transposed", "second_duplicate_dropped", "weak_block_dropped", "inactive_side_added",
             "masked_column_not_skipped", "median_one_too_low", "no_rotation_rule_omitted"]


@pytest.mark.parametrize("kind", MUTATIONS)
def test_comparator_rejects_a_wrong_assembly(oracle_lib, kind):
    ref = _ref(oracle_lib, "graph6")
    err = pp.block_errors(_mutated(ref, kind), ref.S, ref.scale, 6)
    print("%s: worst block %.3g at %s, %d spurious, %d missing (tolerance %.3g)"
          % (kind, err.worst, err.where, len(err.spurious), len(err.missing), pp.TOL_S))
    assert not pp.accepted(err, pp.TOL_S)
    assert err.worst > 10 * pp.TOL_S


def test_whole_matrix_norm_accepts_the_dropped_weak_block(oracle_lib):
    """rel_err(S) < 1e-11, the check of test_pose_graph_unary_binary, passes without the weak loop closure; the
    per-block check at the same number does not."""
    ref = _ref(oracle_lib, "graph6")
    S = _mutated(ref, "weak_block_dropped")
    whole = rel_err(pp.symmetric(S), pp.symmetric(ref.S))
    err = pp.block_errors(S, ref.S, ref.scale, 6)
    print("weak block dropped: whole-matrix rel_err %.3g, worst block %.3g" % (whole, err.worst))
    assert whole < 1e-11 < err.worst


def test_comparator_reports_spurious_and_missing_blocks(oracle_lib):
    ref = _ref(oracle_lib, "graph6")
    opt = pp.natural_rows(ref.case.pa, 6) // 6
    S = np.array(ref.S)
    a, b = opt[1], opt[50]
    assert ref.scale[a, b] == 0
    S[a * 6, b * 6 + 5] = 1e-300
    i, j = sorted((opt[40], opt[7]))
    S[i * 6:i * 6 + 6, j * 6:j * 6 + 6] = 0.0
    err = pp.block_errors(S, ref.S, ref.scale, 6)
    assert err.spurious == [(a, b)] and err.missing == [(i, j)] and not pp.accepted(err, np.inf)


# ---- 3. sample counts of the inertial residuals, host build ---------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


@pytest.mark.parametrize("count", pp.IMU_SAMPLE_COUNTS)
@pytest.mark.parametrize("pose_dim", [9, 15])
def test_imu_blocks_of_the_kernels_at_every_sample_count(oracle_lib, pose_dim, count):
    """ba_hostcheck_imu (single pass) and ba_hostcheck_imu_split (step Jacobians per sample first) on one residual
    of each sample count: bitwise equal, and against the oracle with the tolerances of
    test_imu_residual_blocks_of_the_kernels_match_the_oracle.  The information of the 2-sample residual has no
    defined value (reference()); its residual and Jacobians have."""
    hc = hostcheck_lib()
    ref = _ref(oracle_lib, "imu_samples_%d" % pose_dim)
    sc = ref.case.sc
    i = 6 + pp.IMU_SAMPLE_COUNTS.index(count)
    meas = np.ascontiguousarray(sc.imu_meas[i], dtype=np.float64)
    assert meas.shape == (count, 7)
    o = pp.imu_options(oracle_lib.default_options())
    g = np.asarray(sc.gravity, dtype=np.float64)
    r6 = np.array([o.gyro_sigma ** 2] * 3 + [o.accel_sigma ** 2] * 3)
    rb6 = np.array([o.gyro_bias_sigma ** 2] * 3 + [o.accel_bias_sigma ** 2] * 3)
    p1 = np.concatenate([sc.poses[i], sc.init_vel[i], sc.init_bias[i]]).astype(np.float64)
    p2 = np.concatenate([sc.poses[i + 1], sc.init_vel[i + 1], sc.init_bias[i + 1]]).astype(np.float64)
    out = []
    for fn in (hc.ba_hostcheck_imu, hc.ba_hostcheck_imu_split):
        r15, dz1, dz2, ci = np.zeros(15), np.zeros(225), np.zeros(225), np.zeros(225)
        fn(_dp(p1), _dp(p2), _dp(meas), int(count), _dp(g), _dp(r6), _dp(rb6), int(pose_dim), _dp(r15), _dp(dz1),
           _dp(dz2), _dp(ci))
        out.append((r15, dz1.reshape(15, 15), dz2.reshape(15, 15), ci.reshape(15, 15)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    r15, dz1, dz2, ci = out[0]
    q = ref.case.t.counts[0] + i
    sl = np.s_[:pose_dim, :pose_dim]
    e = (rel_err(r15[:pose_dim], ref.imu_residuals[i, :pose_dim]), rel_err(dz1[sl], ref.dz[q, 0][sl]),
         rel_err(dz2[sl], ref.dz[q, 1][sl]), rel_err(ci[sl], ref.imu_cov_inv_oracle[i][sl]))
    print("PoseSize %d, %d samples: r %.3g, dz1 %.3g, dz2 %.3g, cov_inv %.3g" % ((pose_dim, count) + e))
    assert e[0] < 1e-10 and e[1] < 1e-9 and e[2] < 1e-9
    if i in ref.undefined:
        assert count == 2
    else:
        assert e[3] < 1e-8


# ---- 4. the dogleg denominator and the conditioning -----------------------------------------------------------
def test_numpy_dogleg_denominator_reproduces_the_oracles_step(oracle_lib):
    """With a trust region between the Cauchy point and the Gauss-Newton step the oracle's dogleg step is
    delta_sd + beta (delta_gn - delta_sd), delta_sd = alpha rhs, alpha = |rhs|^2 / j_rhs_sq: the j_rhs_sq of
    posepose_cases (binary information WITHOUT the weight, masked columns and inactive poses dropped) gives the
    oracle's delta_p.  The translation of pose 2 is masked by the oracle itself.  beta as the reference computes it
    (quirk Q3: -(b b) in place of -b).  Bound 1e-9: the one the device's scalar is held to."""
    c = pp.graph6()
    m = np.zeros(len(c.pa), np.uint16)
    m[2] = 0x7
    ref = pp.reference(oracle_lib, c, masks=m, regularize=(2,))
    rhs = ref.rhs_oracle
    gn = pp.run_oracle(oracle_lib, c, regularize=(2,)).delta_p()
    sd = (rhs @ rhs) / ref.j_rhs_sq * rhs
    n_sd, n_gn = np.linalg.norm(sd), np.linalg.norm(gn)
    assert n_sd < n_gn
    trust = np.sqrt(n_sd * n_gn)
    got = pp.run_oracle(oracle_lib, c, regularize=(2,), use_dogleg=1, trust_region_size=trust).delta_p()
    diff = gn - sd
    a, b, cc = diff @ diff, 2 * (diff @ sd), sd @ sd - trust * trust
    assert b * b > 4 * a * cc and a > 1e-10
    beta = (-(b * b) + np.sqrt(b * b - 4 * a * cc)) / (2 * a)
    want = sd + beta * diff
    weighted = np.array(ref.info_dogleg)
    nu, nb, _ = c.t.counts
    weighted[nu:nu + nb] *= c.t.bin_w[:, None, None]
    wrong = pp.j_rhs_sq(ref.terms, 6, ref.dz, weighted, rhs, c.pa, m)
    print("dogleg: |sd| %.3g < trust %.3g < |gn| %.3g; step from the numpy denominator rel_err %.3g; the weighted "
          "denominator differs by %.3g" % (n_sd, trust, n_gn, rel_err(want, got), abs(wrong / ref.j_rhs_sq - 1)))
    assert rel_err(want, got) < 1e-9
    assert abs(wrong / ref.j_rhs_sq - 1) > 1e-3


def test_graph6_stays_under_the_cap_of_the_solve_check(oracle_lib):
    ref = _ref(oracle_lib, "graph6")
    S = pp.symmetric(ref.S_oracle)
    tol = lc.tolerance(S)     # (refuses a bound above 1e-8)
    print("graph6: cond(S) %.3g, bound of the solve check %.3g" % (np.linalg.cond(S), tol))
    assert tol <= 1e-8 and np.isfinite(np.linalg.solve(S, ref.rhs_oracle)).all()
