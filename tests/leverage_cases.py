"""Shared by the leverage tests (test_leverages.py, test_leverages_gpu.py): the dense whitened Jacobian of the
projection residuals, the hat blocks from its thin QR, the full-system form J_a inv(H_full) J_a^T, and the call
into the host restatement (ba_hostcheck_leverages).  numpy only."""
import ctypes

import numpy as np


def natural_rows(pa, D=6):
    opt = np.full(len(pa), -1, dtype=np.int64)
    opt[np.asarray(pa).astype(bool)] = np.arange(int(np.asarray(pa).sum()))
    return opt * D


def dense_jacobian(LM, D, K, pose_active, lm_active, lm_ref, pp, pl, jm, jr, jl, jk=None):
    """J (2 O x (n + K + LM Lact)) from sqrt(w)-weighted per-residual blocks jm, jr (O x 2 x 6), jl (O x 2 x LM) and
    jk (O x 2 x K): columns = active poses in id order (D each), calibration, active landmarks in id order.
    The listing rule: an LM == 1 observation from the landmark's reference pose carries no pose block."""
    O = len(pp)
    rows = natural_rows(pose_active, D)
    lopt = np.full(len(lm_active), -1, dtype=np.int64)
    lopt[np.asarray(lm_active).astype(bool)] = np.arange(int(np.asarray(lm_active).sum()))
    n = int(np.asarray(pose_active).sum()) * D
    nl = int(np.asarray(lm_active).sum()) * LM
    J = np.zeros((2 * O, n + K + nl))
    for a in range(O):
        m, l = int(pp[a]), int(pl[a])
        ref = int(lm_ref[l])
        listed = LM != 1 or m != ref
        if listed and rows[m] >= 0:
            J[2 * a:2 * a + 2, rows[m]:rows[m] + 6] += jm[a]
        if LM == 1 and listed and rows[ref] >= 0:
            J[2 * a:2 * a + 2, rows[ref]:rows[ref] + 6] += jr[a]
        if K:
            J[2 * a:2 * a + 2, n:n + K] += jk[a][:, :K]
        if lopt[l] >= 0:
            J[2 * a:2 * a + 2, n + K + LM * lopt[l]:n + K + LM * (lopt[l] + 1)] += jl[a]
    return J, n + K


def qr_blocks(J):
    """(O, 2, 2) diagonal blocks of Q Q^T for the thin QR of J; columns that are entirely zero (masked
    parameters) are dropped first, they span nothing."""
    J = J[:, np.abs(J).max(0) > 0]
    Q = np.linalg.qr(J)[0]
    Q = Q.reshape(-1, 2, Q.shape[1])
    return np.einsum("aik,ajk->aij", Q, Q)


def reduced_system(J, n):
    """(S, Sigma = inv(S)) of the first n columns, the rest eliminated (V block diagonal by construction)."""
    H = J.T @ J
    U, W, V = H[:n, :n], H[:n, n:], H[n:, n:]
    S = U - W @ np.linalg.solve(V, W.T) if V.size else U
    return S, np.linalg.inv(S)


def full_form(J, H_full, ids):
    """J_a inv(H_full) J_a^T for the residuals ids"""
    out = np.empty((len(ids), 2, 2))
    rows = np.concatenate([[2 * a, 2 * a + 1] for a in ids]).astype(np.int64)
    X = np.linalg.solve(H_full, J[rows].T)
    for q in range(len(ids)):
        out[q] = J[rows[2 * q:2 * q + 2]] @ X[:, 2 * q:2 * q + 2]
    return out


def host_leverages(hc, LM, D, K, pose_active, lm_active, lm_ref, pp, pl, jm, jr, jl, jk, w, sigma, variant=0):
    """ba_hostcheck_leverages: jm, jr, jl (jk) UNWEIGHTED per residual, w the weights -> (O, 2, 2)"""
    def p(a, t):
        return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))
    dbl, u32, u8 = ctypes.c_double, ctypes.c_uint32, ctypes.c_uint8
    c = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
    pa, la, ref = c(pose_active, np.uint8), c(lm_active, np.uint8), c(lm_ref, np.uint32)
    pp, pl = c(pp, np.uint32), c(pl, np.uint32)
    jm, jr, jl, jk, w, sigma = (c(x, np.float64) for x in (jm, jr, jl, jk, w, sigma))
    O = len(pp)
    out = np.full((O, 2, 2), np.nan)
    hc.ba_hostcheck_leverages.restype = ctypes.c_int
    rc = hc.ba_hostcheck_leverages(LM, D, K, len(pa), p(pa, u8), len(la), p(la, u8), p(ref, u32), O, p(pp, u32),
                                   p(pl, u32), p(jm, dbl), p(jr, dbl), p(jl, dbl), p(jk, dbl), p(w, dbl),
                                   p(sigma, dbl), int(variant), p(out, dbl))
    assert rc == 0, rc
    return out


# ---- on the device (imports of the engine kept inside: the CPU suite uses the functions above only) ----------------
EPS = np.finfo(np.float64).eps


class Setup:
    pass


def engine(sc, lm_dim, pa, mode=0, tvs=False, pose_pose=False, calib=0, lm_active=None, obs=None, masks=None,
           perm=None, weight=None):
    """An engine on the scene's accepted residuals (obs = (z, pose, lm) for scenes whose observation table is not
    make_scene's; perm: the permutation of ORDER_USER; weight: per residual), finalized, masks set: the construction tests/test_marginals_gpu.py uses."""
    from ba_amd import hipapi
    from helpers import _add_pose_pose
    eng = hipapi.Engine(lm_dim, 6)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 1
    o.keep_reduced_system = 1
    eng.set_options(o)
    if tvs or calib:
        eng.set_calibration(calib, tvs)
    nsel = (sc.obs_per_landmark or 0) + (1 if lm_dim == 1 else 0)
    if obs is None:
        sel = np.ones(len(sc.obs_pose), dtype=bool)
        if lm_dim == 1:
            sel[::nsel] = False
        z, pose, lm = sc.obs_z[sel], sc.obs_pose[sel], sc.obs_lm[sel]
    else:
        z, pose, lm = obs
    eng.set_cameras(sc.cam_params, [0.01, -0.02, 0.03, 0, 0, 0, 1] if tvs else [0, 0, 0, 0, 0, 0, 1])
    eng.set_poses(sc.poses, is_active=pa)
    eng.set_landmarks(sc.landmarks, sc.lm_ref_pose, is_active=lm_active)
    if calib:
        eng.set_landmark_ref_pixels(sc.obs_z[::nsel])
    eng.set_projection_residuals(z, pose, lm, weight=weight)
    if pose_pose:
        _add_pose_pose(eng, sc, sc.num_poses)
    eng.set_pose_ordering(mode)
    if perm is not None:
        eng.set_pose_permutation(perm)
    s = Setup()
    s.eng, s.sc, s.pa, s.lm_dim = eng, sc, np.asarray(pa, dtype=np.uint8), lm_dim
    s.la = np.ones(sc.num_landmarks, dtype=np.uint8) if lm_active is None else np.asarray(lm_active, dtype=np.uint8)
    s.D, s.K = 6, (6 if tvs else calib)
    s.obs_pose, s.obs_lm = np.asarray(pose, dtype=np.int64), np.asarray(lm, dtype=np.int64)
    s.masks = np.zeros(sc.num_poses, dtype=np.uint16) if masks is None else np.asarray(masks, dtype=np.uint16)
    eng.finalize()
    eng.begin_solve()
    eng.set_pose_masks(s.masks)
    return s


def solve(s):
    s.eng.linearize()
    assert s.eng.solve_gn() == 0


def tolerance(S):
    """DESIGN.md section 8, absolute (|H| <= 1); the scene must keep it at or below 1e-8"""
    tol = max(1e-9, 4.5 * EPS * np.linalg.cond(S))
    assert tol <= 1e-8, "scene too ill-conditioned for the check: %g" % tol
    return tol


def engine_jacobian(s):
    """(J, n + K) of dense_jacobian from the engine's whitened Jacobians of the last linearisation (masked columns
    are zero in them, an inactive landmark's dz_dlm too)"""
    nres = len(s.obs_pose)
    jm, jr, jl, _ = s.eng.get_proj_jacobians(nres)
    jk = s.eng.get_calib_jacobians(nres) if s.K else None
    return dense_jacobian(s.lm_dim, s.D, s.K, s.pa, s.la, s.sc.lm_ref_pose, s.obs_pose, s.obs_lm, jm, jr, jl, jk)


def hfull_form(s, S, J, ids):
    """J_a inv(H_full) J_a^T for the residuals ids, H_full = [[S + W V^-1 W^T, W], [W^T, V]] over the active landmarks
    of those residuals (the others are eliminated exactly: their Schur terms are in S) — S as the engine kept it
    (pose-pose terms, priors and the 1e6 of masked parameters included), W and V from the engine's Jacobians: the
    construction of _landmark_reference in tests/test_marginals_gpu.py."""
    LM, n = s.lm_dim, S.shape[0]
    lopt = np.full(len(s.la), -1, dtype=np.int64)
    lopt[s.la.astype(bool)] = np.arange(int(s.la.sum()))
    lms = sorted({int(s.obs_lm[a]) for a in ids if s.la[s.obs_lm[a]]})
    cols = np.concatenate([n + LM * lopt[l] + np.arange(LM) for l in lms]).astype(np.int64) if lms else np.zeros(0, np.int64)
    Jl = J[:, cols]
    W = J[:, :n].T @ Jl
    V = Jl.T @ Jl
    U = S + W @ np.linalg.solve(V, W.T) if len(cols) else S
    H = np.block([[U, W], [W.T, V]])
    Ja = np.hstack([J[:, :n], Jl])
    return full_form(Ja, H, ids)


def unknowns_seen(s):
    """unknowns that a projection residual touches: unmasked active pose parameters, calibration, and LM per active
    landmark with at least one residual — what the traces of the hat blocks sum to when nothing else constrains"""
    masked = sum(bin(int(m) & 0x3f).count("1") for m, a in zip(s.masks, s.pa) if a)
    seen = np.bincount(s.obs_lm, minlength=len(s.la)) > 0
    return int(s.pa.sum()) * s.D - masked + s.K + s.lm_dim * int((seen & s.la.astype(bool)).sum())
