"""Shared helpers for the parity tests (numpy only)."""
import ctypes
import os

import numpy as np

from ba_amd import scene

u32p = ctypes.POINTER(ctypes.c_uint32)
dp = ctypes.POINTER(ctypes.c_double)
u8p = ctypes.POINTER(ctypes.c_uint8)


def _p(a, t):
    return a.ctypes.data_as(t)


def _add_pose_pose(eng, sc, P, seed=3):
    """unary priors on every 7th pose and binary odometry between neighbours (every 3rd pair)"""
    rng = np.random.default_rng(seed)
    un = np.arange(0, P, 7, dtype=np.uint32)
    cov = np.ascontiguousarray(np.tile(np.diag([1e2] * 3 + [1e3] * 3).reshape(1, 36), (len(un), 1)))
    prior = np.ascontiguousarray(sc.gt_poses[un])
    rot = np.ones(len(un), dtype=np.uint8)
    eng._chk(eng.L.ba_hip_set_unary_residuals(eng.h, len(un), _p(un, u32p), _p(prior, dp), _p(cov, dp), _p(rot, u8p)))
    p1 = np.arange(0, P - 1, 3, dtype=np.uint32)
    p2 = p1 + 1
    nb = len(p1)
    t12 = np.zeros((nb, 7))
    for k, (a, b) in enumerate(zip(p1, p2)):
        Ra = scene.quat_to_rot(sc.gt_poses[a, 3:7])
        t12[k, :3] = Ra.T @ (sc.gt_poses[b, :3] - sc.gt_poses[a, :3]) + 0.01 * rng.normal(size=3)
        t12[k, 3:7] = scene.quat_mul(sc.gt_poses[a, 3:7] * np.array([-1, -1, -1, 1]), sc.gt_poses[b, 3:7])
    ci = np.ascontiguousarray(np.tile(np.diag([50.0] * 6).reshape(1, 36), (nb, 1)))
    cs = np.ascontiguousarray(np.tile(np.diag([np.sqrt(50.0)] * 6).reshape(1, 36), (nb, 1)))
    w = np.ones(nb)
    rot = np.ones(nb, dtype=np.uint8)
    eng._chk(eng.L.ba_hip_set_binary_residuals(eng.h, nb, _p(p1, u32p), _p(p2, u32p), _p(t12, dp), _p(ci, dp),
                                               _p(cs, dp), _p(w, dp), _p(rot, u8p)))


def hostcheck_lib():
    """libba_hostcheck.so (ba_amd/csrc/hostcheck.cpp: host restatements of the device code), built on first use"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "ba_amd", "lib", "libba_hostcheck.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(path)


def gn_options(po, **kw):
    """Options for fixed-count Gauss-Newton runs (exit tests disabled)."""
    o = po.default_options()
    o.use_dogleg = 0
    o.error_change_threshold = 0
    o.param_change_threshold = 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def fill(ba, sc, active=None, lm_active=None):
    ba.AddCamera(sc.cam_params)
    ba.add_poses(sc.poses, v_w=getattr(sc, "init_vel", None), b=getattr(sc, "init_bias", None),
                 is_active=active, time=getattr(sc, "pose_time", None))
    ba.add_landmarks(sc.landmarks, sc.lm_ref_pose, is_active=lm_active)
    return ba.add_projection_residuals(sc.obs_z, sc.obs_pose, sc.obs_lm)


def accepted_obs(sc):
    """(meas pose, ref pose, landmark) per ACCEPTED residual id, in residual-id order."""
    nsel = sc.obs_per_landmark + (1 if sc.lm_dim == 1 else 0)
    out = []
    for i in range(len(sc.obs_pose)):
        if sc.lm_dim == 1 and i % nsel == 0:
            continue  # the reference-frame observation is rejected (BundleAdjuster.h:489-501)
        out.append((int(sc.obs_pose[i]), int(sc.lm_ref_pose[sc.obs_lm[i]]), int(sc.obs_lm[i])))
    return out


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def brute_force_schur(LM, D, pose_active, lm_active, lm_ref, pp, pl, jm, jr, jl, r, w):
    """Dense restatement of the reference's algebra from per-residual Jacobians (tests/test_structure_lists.py):
    -> (S, rhs_p, rhs_sc) over the active poses in id order."""
    P, L, O = len(pose_active), len(lm_active), len(pp)
    popt = -np.ones(P, dtype=int)
    popt[pose_active > 0] = np.arange(int(pose_active.sum()))
    lopt = -np.ones(L, dtype=int)
    lopt[lm_active > 0] = np.arange(int(lm_active.sum()))
    n, nl = int(pose_active.sum()) * D, int(lm_active.sum()) * LM
    Jp, Jl, rr = np.zeros((2 * O, n)), np.zeros((2 * O, max(nl, 1))), np.zeros(2 * O)
    for a in range(O):
        sw = np.sqrt(w[a])
        l, m, ref = pl[a], pp[a], lm_ref[pl[a]]
        listed = LM != 1 or m != ref
        rr[2 * a:2 * a + 2] = sw * r[a]
        if listed and popt[m] >= 0:
            Jp[2 * a:2 * a + 2, popt[m] * D:popt[m] * D + 6] += sw * jm[a].reshape(2, 6)
        if LM == 1 and listed and popt[ref] >= 0:
            Jp[2 * a:2 * a + 2, popt[ref] * D:popt[ref] * D + 6] += sw * jr[a].reshape(2, 6)
        if lopt[l] >= 0:
            Jl[2 * a:2 * a + 2, lopt[l] * LM:lopt[l] * LM + LM] = sw * jl[a].reshape(2, LM)
    U, W = Jp.T @ Jp, Jp.T @ Jl
    V = Jl.T @ Jl
    Vi = np.zeros_like(V)
    for k in range(int(lm_active.sum())):
        blk = V[k * LM:(k + 1) * LM, k * LM:(k + 1) * LM].copy()
        if LM == 1:
            if abs(blk[0, 0]) < 1e-6:
                blk[0, 0] += 1e-6            # BundleAdjuster.cpp:431-434
        elif np.linalg.norm(blk) < 1e-6:
            blk += 1e-6 * np.eye(3)          # :435-439
        Vi[k * LM:(k + 1) * LM, k * LM:(k + 1) * LM] = np.linalg.inv(blk)
    rhs_p = Jp.T @ rr
    rhs_l = Jl.T @ rr
    return U - W @ Vi @ W.T, rhs_p, rhs_p - W @ Vi @ rhs_l


def schur_lists(hc, LM, D, pose_active, lm_active, lm_ref, pp, pl, jm, jr, jl, r, w):
    """ba_hostcheck_schur_lists (ba_amd/csrc/hostcheck.cpp) on one graph: the static lists of ba_hip_finalize, evaluated
    on the CPU as the device kernels evaluate them.  Asserts the library's own range invariants (return code 0) and the
    leading dimension; -> (S symmetric n x n, S_lower as stored, rhs_p, rhs_sc, counts[8])."""
    def p(a, t):
        return a.ctypes.data_as(ctypes.POINTER(t))
    P, L, O = len(pose_active), len(lm_active), len(pp)
    n = int(pose_active.sum()) * D
    ld = max(64, (n + 63) // 64 * 64)
    S_lower, rhs_p, rhs_sc = np.zeros((ld, ld)), np.zeros(ld), np.zeros(ld)
    vinv, bl = np.zeros((L, LM * LM)), np.zeros((L, LM))
    out_ld = ctypes.c_uint32()
    counts = np.zeros(8, dtype=np.uint32)
    dbl, u32, u8 = ctypes.c_double, ctypes.c_uint32, ctypes.c_uint8
    rc = hc.ba_hostcheck_schur_lists(
        LM, D, P, p(pose_active, u8), L, p(lm_active, u8), p(lm_ref, u32), O, p(pp, u32), p(pl, u32),
        p(jm, dbl), p(jr, dbl), p(jl, dbl), p(r, dbl), p(w, dbl), p(S_lower, dbl), p(rhs_p, dbl),
        p(rhs_sc, dbl), p(vinv, dbl), p(bl, dbl), ctypes.byref(out_ld), p(counts, u32))
    assert rc == 0, rc
    assert out_ld.value == ld
    # lower storage -> symmetric: blocks (i < j) are stored transposed below the diagonal, the
    # diagonal D x D blocks with both triangles
    S = np.tril(S_lower[:n, :n], -1)
    S = S + S.T
    for q in range(n // D):
        S[q * D:q * D + D, q * D:q * D + D] = S_lower[q * D:q * D + D, q * D:q * D + D]
    return S, S_lower, rhs_p, rhs_sc, counts
