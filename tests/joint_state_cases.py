"""Shared by the tests of the joint covariances of mixed pose / calibration / landmark sets
(test_joint_state_plan.py, test_joint_state_gpu.py): the error measure in correlation units, the calls into the host
restatement (ba_hostcheck_joint_rhs, ba_hostcheck_joint_state) and the dense references.  numpy only."""
import ctypes

import numpy as np

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
dp = ctypes.POINTER(ctypes.c_double)


def corr_err(got, want):
    """max_ab |got - want|_ab / (d_a d_b), d = sqrt(diag(want)): an error in correlation units, so that neither the
    landmark nor the pose side (variance scales apart by 0.07 to 220) hides the other"""
    d = np.sqrt(np.diag(want))
    assert np.all(d > 0)
    return float((np.abs(got - want) / np.outer(d, d)).max())


def joint_rhs(hc, S, B):
    """ba_hostcheck_joint_rhs: (cov = B^T S^-1 B, Y, reach, level_of, nzL, products, levels)"""
    n = S.shape[0]
    nt = (n + 63) // 64
    S = np.ascontiguousarray(S, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    assert B.shape[0] == n
    m = B.shape[1]
    cov = np.zeros((m, m))
    Y = np.zeros((64 * nt, m))
    reach = np.zeros(nt, dtype=np.uint8)
    level_of = np.zeros(nt, dtype=np.uint32)
    nzL = np.zeros(nt * nt, dtype=np.uint8)
    prod, lev = ctypes.c_uint64(), ctypes.c_uint32()
    hc.ba_hostcheck_joint_rhs.restype = ctypes.c_int
    rc = hc.ba_hostcheck_joint_rhs(n, S.ctypes.data_as(dp), m, B.ctypes.data_as(dp), cov.ctypes.data_as(dp),
                                   Y.ctypes.data_as(dp), reach.ctypes.data_as(u8p), level_of.ctypes.data_as(u32p),
                                   nzL.ctypes.data_as(u8p), ctypes.byref(prod), ctypes.byref(lev))
    assert rc == 0, rc
    return cov, Y, reach.astype(bool), level_of, nzL.reshape(nt, nt), prod.value, lev.value


def host_joint_state(hc, LM, D, K, pose_active, lm_active, lm_ref, pp, pl, jm, jr, jl, jk, w, S, pose_ids, lm_ids,
                     include_calibration=False, variant=0):
    """ba_hostcheck_joint_state: jm, jr, jl (jk) UNWEIGHTED per residual, w the weights, S the dense reduced system
    -> (cov (M, M), reach flags)"""
    def p(a, t):
        return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))
    dbl, u32, u8 = ctypes.c_double, ctypes.c_uint32, ctypes.c_uint8
    c = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
    pa, la, ref = c(pose_active, np.uint8), c(lm_active, np.uint8), c(lm_ref, np.uint32)
    pp, pl = c(pp, np.uint32), c(pl, np.uint32)
    jm, jr, jl, jk, w, S = (c(x, np.float64) for x in (jm, jr, jl, jk, w, S))
    pose_ids, lm_ids = c(np.atleast_1d(pose_ids), np.uint32), c(np.atleast_1d(lm_ids), np.uint32)
    n = S.shape[0]
    M = len(pose_ids) * D + (K if include_calibration else 0) + len(lm_ids) * LM
    cov = np.full((M, M), np.nan)
    reach = np.zeros((n + 63) // 64, dtype=np.uint8)
    hc.ba_hostcheck_joint_state.restype = ctypes.c_int
    rc = hc.ba_hostcheck_joint_state(LM, D, K, len(pa), p(pa, u8), len(la), p(la, u8), p(ref, u32), len(pp), p(pp, u32),
                                     p(pl, u32), p(jm, dbl), p(jr, dbl), p(jl, dbl), p(jk, dbl), p(w, dbl), n,
                                     p(S, dbl), len(pose_ids), p(pose_ids, u32), int(bool(include_calibration)),
                                     len(lm_ids), p(lm_ids, u32), int(variant), p(cov, dbl), p(reach, u8))
    assert rc == 0, rc
    return cov, reach.astype(bool)


def request_columns(LM, D, K, pose_active, lm_active, pose_ids, lm_ids, include_calibration=False):
    """columns of leverage_cases.dense_jacobian (active poses in id order, calibration, active landmarks in id order)
    that a request selects, in the request's order"""
    popt = np.cumsum(np.asarray(pose_active).astype(bool)) - 1
    lopt = np.cumsum(np.asarray(lm_active).astype(bool)) - 1
    n = int(np.asarray(pose_active).astype(bool).sum()) * D
    cols = [popt[p] * D + x for p in pose_ids for x in range(D)]
    if include_calibration:
        cols += [n + x for x in range(K)]
    cols += [n + K + lopt[l] * LM + k for l in lm_ids for k in range(LM)]
    return np.asarray(cols, dtype=np.int64)


def full_inverse_block(H, S_pose, n, lm_cols):
    """inv([[S + W V^-1 W^T, W], [W^T, V]]) over the pose + calibration rows and the landmark columns lm_cols of the
    full normal matrix H (W, V taken from H; S_pose: the reduced system that already holds every landmark's Schur
    term, pose-pose terms and priors): the landmarks not asked for stay eliminated exactly."""
    W = H[:n, lm_cols]
    V = H[np.ix_(lm_cols, lm_cols)]
    U = S_pose + W @ np.linalg.solve(V, W.T) if len(lm_cols) else S_pose
    return np.linalg.inv(np.block([[U, W], [W.T, V]]))
