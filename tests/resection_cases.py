"""Pose refinement (resection) with the landmarks held fixed: an independent numpy Levenberg-Marquardt in float64 and the
case builders, shared by tests/test_resection.py (host restatement ba_hostcheck_refine_poses) and
tests/test_resection_gpu.py (device).

The numpy LM is written from the rules of the feature, not from ba_amd/csrc/resect.h, and is vectorised over the
observations of a pose (so its sums are numpy's, in another order than the restatement's):
  cost       E_p = sum w |z - pi(P)|^2 over every projection residual measured from pose p; vehicle point
             Pp = R_wp^T (X - X_w t_wp), sensor point P = R_vs^T (Pp - X_w t_vs); X the homogeneous world point
  update     t <- t - d[0:3], q <- normalize(q exp(-d[3:6]));  A = -dr/dd = dpi [X_w R_sw | -R_vs^T [Pp]x]
  iteration  H = sum w A^T A, g = sum w A^T r, D = clamp(diag H, 1e-6, 1e32), (H + lambda D) d = g, predicted decrease
             d^T (lambda D d + g), Nielsen's update; fixed parameters leave the system
  cheirality observations at depth <= 0 (or non-finite) at the starting pose are excluded and counted; a trial pose
             with a used observation at depth <= 0 is rejected like a cost increase
  stop       E <= F = sum w (8 eps)^2 |z|^2 (the cost is zero as far as residuals that carry about eight roundings of
             numbers of the size of the pixel can tell; E = 0 is a case of it), or max_i |g_i| / sqrt(H_ii E) <= gradient_tolerance, or an accepted step with
             |dt| <= step_tolerance (|t| + step_tolerance) and |dw| <= step_tolerance
  status     TOO_FEW_OBSERVATIONS (2 used < free parameters), FAILED (non-finite), OK, NOT_CONVERGED (written when the
             cost fell)
`wrong=` switches on one deliberate mistake, for the tests that show the comparison can tell.
Numpy only; the engine is imported inside the functions that need it."""
import ctypes

import numpy as np

import triangulation_cases as tc
from ba_amd import scene

EPS = np.finfo(np.float64).eps
OK, NOT_CONVERGED, TOO_FEW, FAILED = range(4)
DEFAULTS = dict(max_iterations=20, write_back=1, fixed_mask=0, initial_damping=1e-3, gradient_tolerance=1e-6,
                step_tolerance=1e-12, huber_width=0.0)
WRONG = ("rotation_side", "no_tvs", "drop_same_pose", "huber_frozen", "no_trial_cheirality")
# observations per pose at the edges of the kernel: the TOO_FEW boundary, the wave, the block (SLOTS 1), SLOTS 4 /
# streaming, and one pose well inside the streaming kernel
EDGE_COUNTS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1024, 1025, 1100)
SMALL_COUNTS = (0, 2, 3, 40, 65, 130)


def options(**kw):
    o = dict(DEFAULTS)
    for k in kw:
        assert k in o, k
    o.update(kw)
    return o


# ---- small rotations ----------------------------------------------------------------------------------------------
def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def quat_exp(w):
    th = np.linalg.norm(w)
    if th < 1e-10:
        q = np.append(0.5 * np.asarray(w), 1.0)
    else:
        q = np.append(np.sin(0.5 * th) / th * np.asarray(w), np.cos(0.5 * th))
    return q / np.linalg.norm(q)


def rot_from_to(z_axis, roll):
    """a rotation whose third column is z_axis, rolled about it"""
    z = z_axis / np.linalg.norm(z_axis)
    a = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(a, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)
    c, s = np.cos(roll), np.sin(roll)
    return R @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def rot_to_quat(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 1e-3:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:   # (not met by the builders below: they keep the rotation angle below 180 degrees)
        x = np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2.0
        q = np.array([x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x), (R[2, 1] - R[1, 2]) / (4 * x)])
    return q / np.linalg.norm(q)


def angle_between(q, q_true):
    """angle of q^-1 q_true"""
    qi = np.array([-q[0], -q[1], -q[2], q[3]])
    d = quat_mul(qi, q_true)
    return 2.0 * np.arctan2(np.linalg.norm(d[:3]), abs(d[3]))


# ---- the case builders --------------------------------------------------------------------------------------------
def make_case(counts, lm_dim, seed=0, rig=False, fov=False, pose_cam=False, pixel_sigma=0.0, outlier_frac=0.0,
              direction=False):
    """poses on a ring of radius 8 looking at a ball of landmarks (radius 2) with a random roll; pose p measures
    counts[p] landmarks, each once.  Returns (case at the ground truth, true poses).  rig: two cameras with non-identity
    T_vs, alternating; fov: an FOV camera; pose_cam: per-pose intrinsics; outlier_frac: that share of the observations of
    the poses with at least 40 get a far pixel, or a landmark of their own behind the camera; direction: landmark 0 is
    uploaded as a pure direction (far point, X_w = 0)."""
    rng = np.random.default_rng(seed)
    P, L = len(counts), max(max(counts), 8) + 40
    c = tc.Case()
    c.lm_dim = lm_dim
    X = rng.normal(size=(L, 3))
    X = 2.0 * X / np.linalg.norm(X, axis=1, keepdims=True) * rng.uniform(0.2, 1.0, size=(L, 1)) ** (1 / 3)
    poses = np.zeros((P, 7))
    for p in range(P):
        a = rng.uniform(-1.0, 1.0)
        pos = np.array([8.0 * np.sin(a), rng.uniform(-1.0, 1.0), -8.0 * np.cos(a)])
        poses[p, :3] = pos
        poses[p, 3:] = rot_to_quat(rot_from_to(-pos, rng.uniform(-0.5, 0.5)))
    c.poses = poses
    if rig:
        c.cam_params = np.array([[500.0, 505.0, 320.0, 240.0], [420.0, 415.0, 300.0, 250.0]])
        c.cam_tvs = np.array([np.append([0.10, -0.05, 0.02], quat_exp([0.05, -0.1, 0.03])),
                              np.append([-0.20, 0.03, 0.05], quat_exp([-0.04, 0.12, 0.2]))])
    else:
        c.cam_params = np.array([[500.0, 505.0, 320.0, 240.0]])
        c.cam_tvs = np.array([[0.0, 0, 0, 0, 0, 0, 1]])
    C = len(c.cam_params)
    c.cam_model = np.zeros(C, dtype=np.int32)
    c.cam_w = np.zeros(C)
    if fov:
        c.cam_model[:], c.cam_w[:] = 1, 0.9
    c.pose_cam = None
    if pose_cam:
        c.pose_cam = c.cam_params[0] * (1.0 + 0.02 * rng.uniform(-1, 1, size=(P, 4)))
    c.x_w = np.hstack([X, np.ones((L, 1))])
    if direction:
        d = np.array([0.1, -0.05, 1.0])   # (in front of every camera of the ring: they all look towards +z)
        c.x_w[0] = np.append(d / np.linalg.norm(d), 0.0)
    obs_pose, obs_lm, obs_cam = [], [], []
    for p, k in enumerate(counts):
        lms = rng.permutation(L)[:k]
        if direction and k >= 40 and 0 not in lms:
            lms[0] = 0
        obs_pose += [p] * k
        obs_lm += list(lms)
        obs_cam += list((np.arange(k) + p) % C)
    order = rng.permutation(len(obs_pose))   # (the caller's order is not the engine's)
    c.pose = np.array(obs_pose, dtype=np.uint32)[order]
    c.lm = np.array(obs_lm, dtype=np.uint32)[order]
    c.cam = np.array(obs_cam, dtype=np.uint32)[order]
    c.weight = rng.uniform(0.5, 2.0, size=len(order))
    # the reference pose of a landmark: its first observer (pose 0 for a landmark nobody measures)
    c.ref_pose = np.zeros(L, dtype=np.uint32)
    c.ref_cam = np.zeros(L, dtype=np.uint32)
    seen = np.zeros(L, dtype=bool)
    for a in range(len(order)):
        if not seen[c.lm[a]]:
            seen[c.lm[a]], c.ref_pose[c.lm[a]], c.ref_cam[c.lm[a]] = True, c.pose[a], c.cam[a]
    c.lm_active = None
    c.z = np.zeros((len(order), 2))
    for a in range(len(order)):
        Pp = sensor_points(c, c.poses[c.pose[a]], np.array([a]))[0]
        c.z[a] = tc.project(camera(c, c.pose[a], c.cam[a]), Pp)[0]
    c.z += pixel_sigma * rng.normal(size=c.z.shape)
    if outlier_frac > 0:
        big = np.array([counts[p] >= 40 for p in c.pose])
        out = np.nonzero(big & (rng.uniform(size=len(order)) < outlier_frac))[0]
        behind = []
        for i, a in enumerate(out):
            if i % 3 == 2:   # a map point of its own behind the camera of the measuring pose
                R = scene.quat_to_rot(c.poses[c.pose[a], 3:7])
                behind.append(np.append(c.poses[c.pose[a], :3] - R[:, 2] * rng.uniform(1.0, 3.0) + 0.3 * rng.normal(size=3), 1.0))
                c.lm[a] = L + len(behind) - 1
            else:
                c.z[a] += rng.uniform(30.0, 80.0, size=2) * rng.choice([-1, 1], size=2)
        if behind:
            c.x_w = np.vstack([c.x_w, behind])
            c.ref_pose = np.append(c.ref_pose, [c.pose[a] for i, a in enumerate(out) if i % 3 == 2]).astype(np.uint32)
            c.ref_cam = np.append(c.ref_cam, [c.cam[a] for i, a in enumerate(out) if i % 3 == 2]).astype(np.uint32)
    return c, poses.copy()


def perturbed(c, seed=1, dt=0.1, dw=np.radians(3.0)):
    """every pose off by dt metres and dw radians in random directions"""
    rng = np.random.default_rng(seed)
    out = c.copy()
    for p in range(len(c.poses)):
        u, v = rng.normal(size=3), rng.normal(size=3)
        out.poses[p, :3] += dt * u / np.linalg.norm(u)
        out.poses[p, 3:] = quat_mul(c.poses[p, 3:], quat_exp(dw * v / np.linalg.norm(v)))
    return out


def cheirality_trap(seed=5):
    """one pose of 64 observations; one more landmark, of negligible weight, sits 2 cm in front of the camera at the
    perturbed start and behind it at the true pose: an enforcing LM cannot walk to the truth, one that does not enforce
    cheirality on trial poses does"""
    c, true = make_case((64,), 3, seed=seed)
    s = perturbed(c, seed=seed + 1)
    R = scene.quat_to_rot(s.poses[0, 3:7])
    Rt_ = scene.quat_to_rot(true[0, 3:7])
    near = lambda: s.poses[0, :3] + R @ np.array([0.001, -0.002, 0.02])
    if (Rt_.T @ (near() - true[0, :3]))[2] > -0.03:   # make sure the truth has it behind: pull the start back
        s.poses[0, :3] -= R[:, 2] * 0.1
    Xn = near()
    assert (Rt_.T @ (Xn - true[0, :3]))[2] < -0.03
    s.x_w = np.vstack([s.x_w, np.append(Xn, 1.0)])
    s.ref_pose = np.append(s.ref_pose, 0).astype(np.uint32)
    s.ref_cam = np.append(s.ref_cam, 0).astype(np.uint32)
    s.pose = np.append(s.pose, 0).astype(np.uint32)
    s.lm = np.append(s.lm, len(s.x_w) - 1).astype(np.uint32)
    s.cam = np.append(s.cam, 0).astype(np.uint32)
    s.weight = np.append(s.weight, 1e-12)
    s.z = np.vstack([s.z, [330.0, 236.0]])
    return s, true


# ---- cameras and points -------------------------------------------------------------------------------------------
def camera(c, p, cm):
    ip = c.pose_cam[p] if c.pose_cam is not None else c.cam_params[cm]
    return (ip[0], ip[1], ip[2], ip[3], c.cam_w[cm], int(c.cam_model[cm]))


def sensor_points(c, pose7, obs, use_tvs=True):
    """the sensor-frame points of the observations obs at the pose"""
    R, t = scene.quat_to_rot(pose7[3:7]), pose7[:3]
    out = np.zeros((len(obs), 3))
    for i, a in enumerate(obs):
        X = c.x_w[c.lm[a]]
        Pp = R.T @ (X[:3] - X[3] * t)
        if use_tvs:
            tv = c.cam_tvs[c.cam[a]]
            Pp = scene.quat_to_rot(tv[3:7]).T @ (Pp - X[3] * tv[:3])
        out[i] = Pp
    return out


def sorted_order(c):
    """the engine's observation order: by landmark, stable"""
    return np.argsort(c.lm, kind="stable")


def pose_lists(c):
    """numpy's answer for build_pose_obs_lists on the sorted order: (ptr [P + 1], idx [O])"""
    pose_sorted = c.pose[sorted_order(c)]
    idx = np.argsort(pose_sorted, kind="stable").astype(np.uint32)
    ptr = np.zeros(len(c.poses) + 1, dtype=np.uint32)
    np.cumsum(np.bincount(pose_sorted, minlength=len(c.poses)), out=ptr[1:])
    return ptr, idx


# ---- the independent LM -------------------------------------------------------------------------------------------
def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def refine_numpy(c, opts=None, ids=None, wrong=None):
    """-> (res [n, 8], t_wp [n, 7], final): final[i] = dict(H, lam, D, g) at the end point of request i"""
    assert wrong is None or wrong in WRONG
    o = options(**(opts or {}))
    ids = np.arange(len(c.poses)) if ids is None else np.asarray(ids)
    order = sorted_order(c)
    free = np.array([not (o["fixed_mask"] >> i & 1) for i in range(6)])
    res, t7, final = np.zeros((len(ids), 8)), np.zeros((len(ids), 7)), {}
    for row, p in enumerate(ids):
        obs = [a for a in order if c.pose[a] == p]
        if wrong == "drop_same_pose" and c.lm_dim == 1:
            obs = [a for a in obs if c.ref_pose[c.lm[a]] != p]
        held = c.poses[p, :7].copy()
        t7[row] = held
        k = len(obs)
        X = c.x_w[c.lm[obs]] if k else np.zeros((0, 4))
        cams = [camera(c, p, c.cam[a]) for a in obs]
        Rvs = [np.eye(3) if wrong == "no_tvs" else scene.quat_to_rot(c.cam_tvs[c.cam[a], 3:7]) for a in obs]
        tvs = [np.zeros(3) if wrong == "no_tvs" else c.cam_tvs[c.cam[a], :3] for a in obs]
        z, w0 = c.z[obs], c.weight[obs]

        def points(pose):
            R, t = scene.quat_to_rot(pose[3:7]), pose[:3]
            Pp = (X[:, :3] - X[:, 3:4] * t) @ R
            Ps = np.array([Rvs[i].T @ (Pp[i] - X[i, 3] * tvs[i]) for i in range(k)]).reshape(k, 3)
            return R, Pp, Ps

        with np.errstate(all="ignore"):
            _, _, Ps0 = points(held)
            use = np.all(np.isfinite(Ps0), axis=1) & (Ps0[:, 2] > 0) if k else np.zeros(0, dtype=bool)
            used, excluded = int(use.sum()), int(k - use.sum())
            frozen, floor = {}, [0.0]

            def sums(pose, guard):
                R, Pp, Ps = points(pose)
                H, g, E, F, dmin = np.zeros((6, 6)), np.zeros(6), 0.0, 0.0, np.inf
                for i in np.nonzero(use)[0]:
                    uv, dpi = tc.project(cams[i], Ps[i])
                    r = z[i] - uv
                    A = dpi @ np.hstack([X[i, 3] * (R @ Rvs[i]).T, -Rvs[i].T @ _skew(Pp[i])])
                    w = w0[i]
                    if o["huber_width"] > 0:
                        en = np.sqrt((r @ r) * w)
                        if wrong == "huber_frozen":
                            en = frozen.setdefault(i, en)
                        if en > o["huber_width"]:
                            w *= o["huber_width"] / en
                    H += w * A.T @ A
                    g += w * A.T @ r
                    bad = guard and not Ps[i, 2] > 0 and wrong != "no_trial_cheirality"
                    E += np.inf if bad else w * (r @ r)
                    F += w * (8.0 * EPS) ** 2 * (z[i] @ z[i])
                    dmin = min(dmin, Ps[i, 2])
                H[~free, :] = 0
                H[:, ~free] = 0
                g[~free] = 0
                floor[0] = F
                return H, g, E, dmin

            def measure(H, g, E):
                return 0.0 if E == 0 else max(abs(g[i]) / np.sqrt(H[i, i] * E) for i in range(6) if free[i])

            if 2 * used < free.sum():
                res[row] = [TOO_FEW, used, 0, 0, 0, 0, 0, excluded]
                if used:
                    res[row, 5] = sums(held, False)[3]
                continue
            H, g, E, depth = sums(held, False)
            Fx = floor[0]
            if not (np.all(np.isfinite(held)) and np.isfinite(E)):
                res[row] = [FAILED, used, 0, 0, 0, depth, 0, excluded]
                continue
            x, lam, nu, it, E0 = held.copy(), o["initial_damping"], 2.0, 0, E
            while True:
                cg = measure(H, g, E)
                if E <= Fx or cg <= o["gradient_tolerance"]:
                    status = OK
                    break
                if it >= o["max_iterations"]:
                    status = NOT_CONVERGED
                    break
                D = np.diag([tc._clamp(H[i, i]) if free[i] else 0.0 for i in range(6)])
                delta = np.zeros(6)
                try:
                    delta[free] = np.linalg.solve((H + lam * D)[np.ix_(free, free)], g[free])
                except np.linalg.LinAlgError:
                    delta[free] = np.nan
                pred = delta @ (lam * D @ delta + g)
                trial = x.copy()
                trial[:3] = x[:3] - delta[:3]
                if free[3:].any():
                    e = quat_exp(-delta[3:])
                    q = quat_mul(e, x[3:]) if wrong == "rotation_side" else quat_mul(x[3:], e)
                    trial[3:] = q / np.linalg.norm(q)
                Ht, gt, Et, dt_ = sums(trial, True)
                Ft = floor[0]
                lam, nu, accept = tc._nielsen(lam, nu, (E - Et) / pred)
                it += 1
                if accept:
                    x, H, g, E, depth, Fx = trial, Ht, gt, Et, dt_, Ft
                    st = o["step_tolerance"]
                    if st > 0 and np.linalg.norm(delta[:3]) <= st * (np.linalg.norm(x[:3]) + st) and np.linalg.norm(delta[3:]) <= st:
                        cg = measure(H, g, E)
                        status = OK
                        break
            res[row] = [status, used, it, E0, E, depth, cg, excluded]
            final[row] = dict(H=H.copy(), lam=lam, D=np.diag([tc._clamp(H[i, i]) if free[i] else 0.0 for i in range(6)]), g=g.copy())
            if status == OK or E < E0:
                t7[row] = x
    return res, t7, final


def pose_bounds(H, lam, t, step_tolerance, fixed_mask=0):
    """(translation bound, rotation bound) of one pose: 2 step_tolerance s + 8 cond2(H + lambda D) eps s with s = |t| + 1
    and s = 1, over the free parameters, D = clamp(diag H)"""
    free = np.array([not (fixed_mask >> i & 1) for i in range(6)])
    D = np.diag([tc._clamp(H[i, i]) for i in range(6)])
    k = np.linalg.cond((H + lam * D)[np.ix_(free, free)])
    s = np.linalg.norm(t) + 1.0
    return 2.0 * step_tolerance * s + 8.0 * k * EPS * s, 2.0 * step_tolerance + 8.0 * k * EPS


# ---- the host restatement (ba_hostcheck_refine_poses) -----------------------------------------------------------------
def refine_host(hc, c, opts=None, ids=None):
    """-> (res [n, 8], t_wp [n, 7], info [n, 6, 6], final [n, 7] = lambda, g) or the message of the refusal"""
    o = options(**(opts or {}))
    order = sorted_order(c)
    f64, u32 = np.float64, np.uint32
    con = lambda a, t: np.ascontiguousarray(a, dtype=t)
    pose, cam, lm = con(c.pose[order], u32), con(c.cam[order], u32), con(c.lm[order], u32)
    z, w = con(c.z[order], f64), con(c.weight[order], f64)
    opts7 = np.array([o[k] for k in ("max_iterations", "write_back", "fixed_mask", "initial_damping", "gradient_tolerance",
                                     "step_tolerance", "huber_width")], dtype=f64)
    ida = None if ids is None else con(ids, u32)
    n = len(c.poses) if ida is None else len(ida)
    m = max(n, 1)
    res, t7, info, final = np.zeros((m, 8)), np.zeros((m, 7)), np.zeros((m, 6, 6)), np.zeros((m, 7))
    msg = ctypes.create_string_buffer(512)
    dbl, U32 = ctypes.c_double, ctypes.c_uint32
    poses = con(c.poses[:, :7], f64)
    pose_cam = None if c.pose_cam is None else con(c.pose_cam, f64)
    P = tc._ptr
    hc.ba_hostcheck_refine_poses.restype = ctypes.c_int
    rc = hc.ba_hostcheck_refine_poses(
        U32(len(poses)), P(poses, dbl), U32(len(c.cam_params)), P(con(c.cam_params, f64), dbl), P(con(c.cam_tvs, f64), dbl),
        P(con(c.cam_model, np.int32), ctypes.c_int32), P(con(c.cam_w, f64), dbl), P(pose_cam, dbl), U32(len(pose)),
        P(pose, U32), P(cam, U32), P(lm, U32), P(z, dbl), P(w, dbl), P(con(c.x_w, f64), dbl), U32(n), P(ida, U32),
        P(opts7, dbl), P(res, dbl), P(t7, dbl), P(info, dbl), P(final, dbl), msg, U32(512))
    assert rc in (0, 1), rc
    if rc:
        return msg.value.decode()
    return res[:n], t7[:n], info[:n], final[:n]


def engine(c, pose_dim=6, v_w=None, b=None):
    """a hipapi.Engine on the case, finalized"""
    from ba_amd import hipapi
    eng = hipapi.Engine(c.lm_dim, pose_dim)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 0
    eng.set_options(o)
    eng.set_cameras(c.cam_params, c.cam_tvs)
    if c.cam_model.any():
        eng.set_camera_models(c.cam_model, c.cam_w)
    pa = np.ones(len(c.poses), dtype=np.uint8)
    pa[0] = 0
    eng.set_poses(c.poses, v_w=v_w, b=b, is_active=pa)
    eng.set_landmarks(c.x_w, c.ref_pose, ref_cam=c.ref_cam, is_active=c.lm_active)
    eng.set_projection_residuals(c.z, c.pose, c.lm, cam=c.cam, weight=c.weight)
    if c.pose_cam is not None:
        eng.set_pose_cam_params(c.pose_cam)
    eng.finalize()
    return eng
