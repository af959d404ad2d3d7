"""The pose-pose residual assembly on the MI355X, block by block (k_posepose.hip with the scatter lists of
engine.hip), on the edge-case graphs of posepose_cases.py and read through the existing taps only: ba_hip_get_S /
get_rhs / get_delta_gn, the error sums of ba_hip_linearize and ba_hip_eval_residuals, ba_hip_dogleg_terms,
ba_hip_get_unary_scales, ba_hip_get_imu_residuals / get_imu_errors and ba_hip_debug_set key 6.

With LmSize 0 every D x D block of S is a small sum of residual blocks.  Each block is compared with the numpy sum
over the oracle's Jacobians AND with the oracle's own S, relative to the block's own scale (the sum of the
magnitudes of its terms): 1e-11 for the pose graphs and 1e-10 for their gradient (the bounds
test_pose_graph_unary_binary applies to the whole matrix), 1e-9 for the inertial case (test_visual_inertial).
test_pose_pose_blocks.py checks the reference itself and that the comparator rejects wrong assemblies."""
import ctypes
import types

import numpy as np
import pytest

from ba_amd import hipapi
from helpers import rel_err
import leverage_cases as lc
import posepose_cases as pp

pytestmark = pytest.mark.gpu

dp, u32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
CAMERA = (np.array([[500.0, 500.0, 320.0, 240.0]]), [0, 0, 0, 0, 0, 0, 1])
# graph6_ordered: the reversed ba_hip_set_pose_permutation; graph6_auto: the tile-aware ordering the engine chooses
GRAPHS = [("graph6", 0), ("graph6", 1), ("graph6_ordered", 0), ("graph6_ordered", 1), ("graph6_auto", 0), ("graph6_auto", 1)]
graphs = pytest.mark.parametrize("name,use_dogleg", GRAPHS)


def _scales(eng, n):
    s = np.ones(max(n, 1))
    eng._chk(eng.L.ba_hip_get_unary_scales(eng.h, s.ctypes.data_as(dp)))
    return s[:n]


# ---- the pose graphs ------------------------------------------------------------------------------------------
_runs = {}


def _graph_run(po, name, use_dogleg):
    """One engine per (case, driver), everything read once: linearise, (dogleg terms,) solve, dogleg terms, evaluate,
    linearise again.  use_dogleg = 1 takes the steepest-descent denominator BEFORE the factorisation, as the
    dogleg iteration of ba::BundleAdjuster does, and again after it (the reused sum); 0 only after it."""
    key = (name, use_dogleg)
    if key in _runs:
        return _runs[key]
    ref = pp.cached_reference(po, "graph6", pp.graph6)
    c = ref.case
    eng = hipapi.Engine(0, 6)
    o = hipapi.Options()
    o.keep_reduced_system = 1
    eng.set_options(o)
    eng.set_cameras(*CAMERA)
    eng.set_poses(c.sc.poses, is_active=c.pa)
    pp.add_to_engine(eng, ref.terms)
    n_act = int(c.pa.sum())
    if name == "graph6_ordered":     # reversed: the opt ids, which `other < j` of the scatter compares, swap sides
        eng.set_pose_ordering(hipapi.ORDER_USER)
        eng.set_pose_permutation(np.arange(n_act, dtype=np.uint32)[::-1])
    elif name == "graph6_auto":
        eng.set_pose_ordering(hipapi.ORDER_AUTO)
    eng.finalize()
    r = types.SimpleNamespace(ref=ref, perm=eng.get_pose_ordering()[0].copy())
    eng.begin_solve()
    eng.set_pose_masks(c.masks)
    r.built = eng.linearize()
    r.scales = _scales(eng, c.t.counts[0])
    r.S_before = eng.get_S()
    r.rhs_sc, r.rhs_p, _ = eng.get_rhs()
    r.sd_before = eng.dogleg_terms(0).j_rhs_sq if use_dogleg else None
    assert eng.solve_gn() == 0
    r.S = eng.get_S()
    r.delta_gn = eng.get_delta_gn()[0]
    r.j_rhs_sq = eng.dogleg_terms(1).j_rhs_sq
    r.evaluated = eng.eval_residuals()
    r.built2 = eng.linearize()
    r.scales2 = _scales(eng, c.t.counts[0])
    r.S2 = eng.get_S()
    eng.close()
    _runs[key] = r
    return r


@graphs
def test_S_per_block(oracle_lib, name, use_dogleg):
    r = _graph_run(oracle_lib, name, use_dogleg)
    ref = r.ref
    n_act = int(ref.case.pa.sum())
    # the outputs are in natural order whatever the engine factorises in
    if name == "graph6_auto":
        assert sorted(r.perm.tolist()) == list(range(n_act))
    else:
        assert np.array_equal(r.perm, np.arange(n_act)[::-1] if name == "graph6_ordered" else np.arange(n_act))
    assert np.array_equal(r.S, r.S_before), "the kept copy of S is not the assembled one"
    e_np = pp.block_errors(r.S, ref.S, ref.scale, 6)
    e_or = pp.block_errors(r.S, ref.S_oracle, ref.scale, 6)
    print("%s dogleg %d: S per block against the numpy sum %.3g at %s, against the oracle %.3g at %s (tolerance %.3g)"
          % (name, use_dogleg, e_np.worst, e_np.where, e_or.worst, e_or.where, pp.TOL_S))
    assert not e_np.spurious and not e_np.missing and not e_or.spurious and not e_or.missing
    assert e_np.worst <= pp.TOL_S and e_or.worst <= pp.TOL_S


@graphs
def test_gradient_per_block(oracle_lib, name, use_dogleg):
    r = _graph_run(oracle_lib, name, use_dogleg)
    ref = r.ref
    e = pp.vector_block_error(r.rhs_sc, ref.rhs_oracle, ref.rhs_scale, 6)
    print("%s dogleg %d: gradient per block against the oracle %.3g (tolerance %.3g)" % (name, use_dogleg, e, pp.TOL_RHS))
    assert e <= pp.TOL_RHS
    assert np.array_equal(r.rhs_p, r.rhs_sc)     # (no landmarks: nothing is eliminated)


@graphs
def test_masked_rows_and_absent_pairs_are_exact(oracle_lib, name, use_dogleg):
    r = _graph_run(oracle_lib, name, use_dogleg)
    c = r.ref.case
    rows = pp.natural_rows(c.pa, 6)
    masked = [rows[p] + k for p in np.nonzero(c.masks)[0] for k in range(6) if (int(c.masks[p]) >> k) & 1]
    assert len(masked) == 6
    for i in masked:
        want = np.zeros(r.S.shape[0])
        want[i] = pp.MASK_DIAGONAL
        assert np.array_equal(r.S[i], want) and np.array_equal(r.S[:, i], want) and r.rhs_sc[i] == 0.0
    absent = r.ref.scale == 0
    assert absent.sum() > 1000
    blocks = np.abs(r.S).reshape(len(absent), 6, len(absent), 6).max(axis=(1, 3))
    assert not blocks[absent].any(), "a block of a pair no residual ties is not exactly zero"
    print("%s dogleg %d: %d masked rows and columns and %d absent blocks exact" % (name, use_dogleg, len(masked), absent.sum()))


@graphs
def test_error_sums_and_unary_scales(oracle_lib, name, use_dogleg):
    r = _graph_run(oracle_lib, name, use_dogleg)
    ref = r.ref
    # (the binary sum of BuildProblem is not the one of EvaluateResiduals: posepose_cases.reference)
    pairs = [(r.built.unary_error, ref.built_unary_error), (r.built.binary_error, ref.built_binary_error),
             (r.evaluated.unary_error, ref.unary_error), (r.evaluated.binary_error, ref.binary_error)]
    worst = max(abs(got - want) / want for got, want in pairs)
    e_s = np.abs(r.scales - ref.un_scale).max()
    down = int((r.scales < 1).sum())
    # a second linearisation at the same state: the weights compound (quirk Q4), as the oracle's cov_inv after a
    # second Solve(1)
    ref2 = pp.cached_reference(oracle_lib, "graph6 twice", pp.graph6, solves=2)
    e_s2 = np.abs(r.scales2 - ref2.un_scale).max()
    e_u2 = abs(r.built2.unary_error - ref2.unary_error) / ref2.unary_error
    e_S2 = pp.block_errors(r.S2, ref2.S_oracle, ref2.scale, 6)
    print("%s dogleg %d: error sums %.3g, unary scales %.3g (%d of %d below 1); second linearisation: scales %.3g, "
          "unary error %.3g, S per block %.3g" % (name, use_dogleg, worst, e_s, down, len(r.scales), e_s2, e_u2, e_S2.worst))
    assert worst <= 1e-8
    assert e_s <= 1e-12 and 0.05 * len(r.scales) <= down <= 0.5 * len(r.scales)
    assert np.abs(ref2.un_scale - ref.un_scale).max() > 1e-3, "the second pass changes nothing"
    assert e_s2 <= 1e-12 and e_u2 <= 1e-8 and pp.accepted(e_S2, pp.TOL_S)


@graphs
def test_dogleg_denominator(oracle_lib, name, use_dogleg):
    r = _graph_run(oracle_lib, name, use_dogleg)
    e = abs(r.j_rhs_sq - r.ref.j_rhs_sq) / r.ref.j_rhs_sq
    print("%s dogleg %d: j_rhs_sq %.12g against numpy %.12g: %.3g" % (name, use_dogleg, r.j_rhs_sq, r.ref.j_rhs_sq, e))
    assert e <= 1e-9
    if use_dogleg:
        assert r.sd_before == r.j_rhs_sq, "the sum reused after the factorisation is not the one taken before it"


@graphs
def test_solve_on_the_engines_own_S(oracle_lib, name, use_dogleg):
    """delta_gn against numpy on the engine's own S: the far loop closures are alone in their off-band tiles, so a
    tile the pattern misses shows here and nowhere else"""
    r = _graph_run(oracle_lib, name, use_dogleg)
    S = pp.symmetric(r.S)
    tol = lc.tolerance(S)
    e = rel_err(r.delta_gn, np.linalg.solve(S, r.rhs_sc))
    print("%s dogleg %d: delta_gn against numpy.linalg.solve %.3g (bound %.3g)" % (name, use_dogleg, e, tol))
    assert e <= tol


# ---- inertial residuals with 2 .. 131 samples -----------------------------------------------------------------
def _imu_run(po, ref, variant):
    c = ref.case
    eng = hipapi.Engine(0, c.D)
    o = hipapi.Options()
    src = pp.imu_options(po.default_options())
    for k in ("gyro_sigma", "accel_sigma", "gyro_bias_sigma", "accel_bias_sigma", "use_robust_norm_for_inertial_residuals"):
        setattr(o, k, getattr(src, k))
    eng.set_options(o)
    eng.set_cameras(*CAMERA)
    eng._chk(eng.L.ba_hip_set_gravity(eng.h, np.ascontiguousarray(c.sc.gravity, dtype=np.float64).ctypes.data_as(dp)))
    eng.set_poses(c.sc.poses, v_w=c.sc.init_vel, b=c.sc.init_bias, is_active=c.pa)
    pp.add_to_engine(eng, ref.terms)
    ni = c.t.counts[2]
    ptr = np.zeros(ni + 1, np.uint32)
    ptr[1:] = np.cumsum([len(m) for m in c.sc.imu_meas])
    m7 = np.ascontiguousarray(np.concatenate(c.sc.imu_meas))
    p1, p2, w = np.ascontiguousarray(c.t.imu_p1), np.ascontiguousarray(c.t.imu_p2), np.ones(ni)
    eng._chk(eng.L.ba_hip_set_imu_residuals(eng.h, ni, p1.ctypes.data_as(u32p), p2.ctypes.data_as(u32p),
                                            ptr.ctypes.data_as(u32p), m7.ctypes.data_as(dp), w.ctypes.data_as(dp)))
    eng.debug_set(6, variant)
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(c.masks)
    r = types.SimpleNamespace()
    r.built = eng.linearize()
    r.S = eng.get_S()
    r.rhs = eng.get_rhs()[0]
    r.evaluated = eng.eval_residuals()
    r.residuals, r.errors = np.zeros((ni, 15)), np.zeros(ni)
    eng._chk(eng.L.ba_hip_get_imu_residuals(eng.h, r.residuals.ctypes.data_as(dp)))
    eng._chk(eng.L.ba_hip_get_imu_errors(eng.h, r.errors.ctypes.data_as(dp)))
    eng.close()
    return r


@pytest.mark.parametrize("pose_dim", [15, 9])
def test_imu_sample_counts(oracle_lib, pose_dim):
    """69 inertial residuals of 2, 3, 11, 64, 65 and 131 samples under every form of the inertial linearisation
    (debug key 6: -1 by count, 0 lane per sample and per residual, 1 a wavefront per residual, 2 single pass, 4 a
    wavefront per sample): S and the gradient per block and the residual vectors against the oracle, the
    per-residual errors against r^T cov_inv r in numpy (1e-8: what the information itself is held to in
    test_hostcheck.py), and the forms against each other.  A 2-sample residual has a residual vector and Jacobians
    but no defined information (posepose_cases.reference): its blocks and its error are left out, nothing else."""
    D = pose_dim
    ref = pp.cached_reference(oracle_lib, "imu_samples_%d" % D, lambda: pp.imu_samples(D))
    ni = ref.case.t.counts[2]
    defined = np.array([i not in ref.undefined for i in range(ni)])
    assert defined.sum() == 57 and ni == 69
    cond = [i for i in range(ni) if not ref.case.pa[i] and ref.case.pa[i + 1]]
    assert cond == [0, 7] and defined[7], "no conditioning residual with a defined information"
    runs = {}
    for v in pp.IMU_VARIANTS:
        r = runs[v] = _imu_run(oracle_lib, ref, v)
        e_np = pp.block_errors(r.S, ref.S, ref.scale, D, ref.undefined_blocks)
        e_or = pp.block_errors(r.S, ref.S_oracle, ref.scale, D, ref.undefined_blocks)
        e_g = pp.vector_block_error(r.rhs, ref.rhs_oracle, ref.rhs_scale, D, ref.undefined_poses)
        e_r = max(rel_err(r.residuals[i, :D], ref.imu_residuals[i, :D]) for i in range(ni))
        e_e = np.abs(r.errors[defined] / ref.imu_errors[defined] - 1).max()
        e_u = max(abs(g.unary_error - ref.unary_error) / ref.unary_error for g in (r.built, r.evaluated))
        print("PoseSize %d, form %2d: S per block against numpy %.3g, against the oracle %.3g at %s; gradient %.3g; "
              "residual vectors %.3g; errors %.3g; unary error %.3g"
              % (D, v, e_np.worst, e_or.worst, e_or.where, e_g, e_r, e_e, e_u))
        assert pp.accepted(e_np, pp.TOL_IMU) and pp.accepted(e_or, pp.TOL_IMU)
        assert e_g <= pp.TOL_IMU and e_r <= 1e-10 and e_e <= 1e-8 and e_u <= 1e-8
    base = runs[2]
    for v in pp.IMU_VARIANTS:
        if v == 2:
            continue
        r = runs[v]
        e_S = pp.block_errors(r.S, base.S, ref.scale, D, ref.undefined_blocks)
        e_g = pp.vector_block_error(r.rhs, base.rhs, ref.rhs_scale, D, ref.undefined_poses)
        e_e = np.abs(r.errors[defined] / base.errors[defined] - 1).max()
        print("PoseSize %d, form %2d against the single pass: S per block %.3g, gradient %.3g, errors %.3g"
              % (D, v, e_S.worst, e_g, e_e))
        assert pp.accepted(e_S, 1e-12) and e_g <= 1e-12 and e_e <= 1e-12
        assert np.array_equal(r.residuals, base.residuals)     # (mode 2 of k_imu whatever the form)
