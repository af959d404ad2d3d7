"""Landmark triangulation with the poses held fixed: a numpy restatement of the rules and the case builders, shared by
tests/test_triangulation.py (host restatement ba_hostcheck_triangulate) and tests/test_triangulation_gpu.py (device).

The restatement is written from the rules of the feature, not from ba_amd/csrc/triang.h:
  tables     T_ws = T_wp T_vs, T_sw its inverse; pinhole and FOV cameras, per-pose intrinsics, the original weights
  LmSize 3   linear: centre c_a = t_ws, bearing d_a = R_ws unit(unproject(z_a)); X = (sum w (I - d d^T))^-1 sum w (I - d d^T) c_a
  LmSize 1   the ray is unit(T_sw(ref) x_w); with T = T_sw_m T_ws_r = (R, t), b = unit(unproject(z)):
             rho = -sum w (b x R r).(b x t) / sum w |b x t|^2
  refine     Levenberg-Marquardt on E = sum w |z - pi(P)|^2 over the landmark's parameters: V = sum w Jl^T Jl,
             b_l = sum w Jl^T r, d = clamp(diag V, 1e-6, 1e32), (V + lambda diag d) delta = b_l, x <- x - delta, predicted
             decrease delta^T (lambda D delta + b_l), Nielsen's update; a step to depth <= 0 in an observing sensor is
             rejected like a cost increase; Huber weights from the current residual norm
  stop       E = 0, or c = max_i |b_i| / sqrt(V_ii E) <= gradient_tolerance, or an accepted |delta| <= step_tolerance (|x| + step_tolerance)
  parallax   the largest angle between the first bearing and any other; LmSize 1: the first is the reference ray
  depth      P.z in the observing sensor (LmSize 1: of the point scaled by rho)
  status     TOO_FEW_VIEWS (fewer than 2 observations or no baseline), FAILED (non-finite), LOW_PARALLAX, BEHIND_CAMERA
             (depth <= 0 at the start), OK, NOT_CONVERGED (written when the cost fell; with the linear start also when it
             did not rise)
Numpy only; the engine is imported inside the functions that need it."""
import ctypes

import numpy as np

from ba_amd import scene

EPS = np.finfo(np.float64).eps
OK, NOT_CONVERGED, TOO_FEW_VIEWS, LOW_PARALLAX, BEHIND_CAMERA, FAILED = range(6)
NAMES = ("OK", "NOT_CONVERGED", "TOO_FEW_VIEWS", "LOW_PARALLAX", "BEHIND_CAMERA", "FAILED")
DEFAULTS = dict(linear_init=1, max_iterations=20, write_back=1, lambda0=1e-3, gradient_tolerance=1e-6, step_tolerance=1e-12,
                min_parallax=0.0, huber_width=0.0)
BASELINE_REL = 1e-12


class Case:
    """One problem: lm_dim; poses [P,7]; cam_params [C,4], cam_tvs [C,7], cam_model [C], cam_w [C]; pose_cam [P,4] or
    None; x_w [L,4], ref_pose, ref_cam [L]; lm_active [L] or None; the residuals z [O,2], pose, cam, lm, weight [O]"""

    def copy(self):
        c = Case()
        c.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()})
        return c


def options(**kw):
    o = dict(DEFAULTS)
    for k in kw:
        assert k in o, k
    o.update(kw)
    return o


def case_from_scene(sc, lm_dim, obs=None, x_w=None):
    """the accepted residuals of a make_scene scene (obs = (z, pose, lm) for another observation table), one pinhole
    camera mounted at the identity, unit weights"""
    c = Case()
    c.lm_dim = lm_dim
    c.poses = np.ascontiguousarray(sc.poses, dtype=np.float64)
    c.cam_params = np.ascontiguousarray(sc.cam_params, dtype=np.float64).reshape(1, -1)[:, :4].copy()
    c.cam_tvs = np.array([[0.0, 0, 0, 0, 0, 0, 1]])
    c.cam_model = np.zeros(1, dtype=np.int32)
    c.cam_w = np.zeros(1)
    if np.size(sc.cam_params) == 5:
        c.cam_model[0], c.cam_w[0] = 1, np.ravel(sc.cam_params)[4]
    c.pose_cam = None
    c.x_w = np.ascontiguousarray(sc.landmarks if x_w is None else x_w, dtype=np.float64).copy()
    c.ref_pose = np.ascontiguousarray(sc.lm_ref_pose, dtype=np.uint32)
    c.ref_cam = np.zeros(len(c.ref_pose), dtype=np.uint32)
    c.lm_active = None
    if obs is None:
        nsel = sc.obs_per_landmark + (1 if lm_dim == 1 else 0)
        sel = np.ones(len(sc.obs_pose), dtype=bool)
        if lm_dim == 1:
            sel[::nsel] = False
        obs = sc.obs_z[sel], sc.obs_pose[sel], sc.obs_lm[sel]
    c.z = np.ascontiguousarray(obs[0], dtype=np.float64)
    c.pose = np.ascontiguousarray(obs[1], dtype=np.uint32)
    c.lm = np.ascontiguousarray(obs[2], dtype=np.uint32)
    c.cam = np.zeros(len(c.pose), dtype=np.uint32)
    c.weight = np.ones(len(c.pose))
    return c


def exact_scene(P, L, k, lm_dim, seed):
    """noise-free: true pixels, ground-truth poses, ground-truth landmarks"""
    return scene.make_scene(P, L, k, lm_dim=lm_dim, seed=seed, pixel_sigma=0.0, outlier_frac=0.0, trans_sigma=0.0,
                            rot_sigma=0.0, depth_sigma=0.0)


def directions_only(c):
    """the landmarks as a tracker without depth has them: LmSize 1 pure directions (w = 0) through the reference
    sensor, LmSize 3 points at a fixed wrong range (5 units along the same ray)"""
    out = c.copy()
    tws, tsw = tables(c)
    for l in range(len(c.x_w)):
        R, t = tws[c.ref_pose[l]][c.ref_cam[l]]
        Rs, ts = tsw[c.ref_pose[l]][c.ref_cam[l]]
        p = Rs @ c.x_w[l, :3] + ts * c.x_w[l, 3]
        ray = p / np.linalg.norm(p)
        out.x_w[l] = np.append(R @ ray, 0.0) if c.lm_dim == 1 else np.append(R @ (5.0 * ray) + t, 1.0)
    return out


# ---- cameras and tables -------------------------------------------------------------------------------------------
def tables(c):
    """tws[p][cam] = (R, t) of T_ws = T_wp T_vs, tsw the inverse"""
    tws, tsw = [], []
    for p in range(len(c.poses)):
        Rp, tp = scene.quat_to_rot(c.poses[p, 3:7]), c.poses[p, :3]
        a, b = [], []
        for k in range(len(c.cam_tvs)):
            Rv, tv = scene.quat_to_rot(c.cam_tvs[k, 3:7]), c.cam_tvs[k, :3]
            R, t = Rp @ Rv, Rp @ tv + tp
            a.append((R, t))
            b.append((R.T, -R.T @ t))
        tws.append(a)
        tsw.append(b)
    return tws, tsw


def _fov(w, r):
    """f = r_d / r_u and df/dr of the FOV model (Devernay & Faugeras), with the limits of the engine's restatement"""
    if w * w <= 1e-5:
        return 1.0, 0.0
    m = 2.0 * np.tan(0.5 * w)
    if r * r < 1e-5:
        return m / w, 0.0
    at, den = np.arctan(r * m), 1.0 + r * r * m * m
    return at / (r * w), m / (den * r * w) - at / (r * r * w)


def _fov_inv(w, rd):
    if w * w <= 1e-5:
        return 1.0
    m = 2.0 * np.tan(0.5 * w)
    if rd * rd < 1e-5:
        return w / m
    return np.tan(rd * w) / (rd * m)


def project(cam, P):
    """pixel and its 2 x 3 derivative; cam = (fx, fy, u0, v0, w, model)"""
    fx, fy, u0, v0, w, model = cam
    px, py = P[0] / P[2], P[1] / P[2]
    dn = np.array([[1.0 / P[2], 0.0, -px / P[2]], [0.0, 1.0 / P[2], -py / P[2]]])   # d (px, py) / dP
    A = np.eye(2)
    f = 1.0
    if model:
        r = np.hypot(px, py)
        f, dr = _fov(w, r)
        k = dr / r if r > 0 else 0.0
        A = f * np.eye(2) + k * np.outer([px, py], [px, py])
    uv = np.array([fx * f * px + u0, fy * f * py + v0])
    return uv, np.diag([fx, fy]) @ A @ dn


def bearing(cam, z):
    fx, fy, u0, v0, w, model = cam
    x, y = (z[0] - u0) / fx, (z[1] - v0) / fy
    if model:
        g = _fov_inv(w, np.hypot(x, y))
        x, y = x * g, y * g
    b = np.array([x, y, 1.0])
    return b / np.linalg.norm(b)


def _angle(a, b):
    return np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)


def _clamp(h):
    return min(max(h, 1e-6), 1e32)


def _nielsen(lam, nu, rho):
    if rho > 0.0:
        return min(max(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e-12), 1e12), 2.0, True
    return min(max(lam * nu, 1e-12), 1e12), 2.0 * nu, False


# ---- the restatement ----------------------------------------------------------------------------------------------
def triangulate_numpy(c, opts=None, ids=None):
    """-> (res [L, 8] with status -1 in rows that were not requested, x_w [L, 4], final): final[l] = (V, lambda, D, x,
    iterations) of landmark l at its end point, for the landmarks that were refined"""
    o = options(**(opts or {}))
    LM, L = c.lm_dim, len(c.x_w)
    tws, tsw = tables(c)
    order = np.argsort(c.lm, kind="stable")
    res = np.zeros((L, 8))
    res[:, 0] = -1
    xw = c.x_w.copy()
    final = {}
    want = np.ones(L, dtype=bool) if ids is None else np.isin(np.arange(L), ids)
    by_lm = [[] for _ in range(L)]
    for a in order:
        by_lm[c.lm[a]].append(a)
    for l in range(L):
        if not want[l]:
            continue
        obs = by_lm[l]
        k = len(obs)
        res[l] = [TOO_FEW_VIEWS, k, 0, 0, 0, 0, 0, 0]
        if k == 0:
            res[l, 1] = 0
            continue
        cams, Ts, zs, ws = [], [], [], []
        Rwr, twr = tws[c.ref_pose[l]][c.ref_cam[l]]
        Rsr, tsr = tsw[c.ref_pose[l]][c.ref_cam[l]]
        for a in obs:
            pm, cm = c.pose[a], c.cam[a]
            ip = c.pose_cam[pm] if c.pose_cam is not None else c.cam_params[cm]
            cams.append((ip[0], ip[1], ip[2], ip[3], c.cam_w[cm], int(c.cam_model[cm])))
            R, t = tsw[pm][cm]
            if LM == 1:
                R, t = R @ Rwr, R @ twr + t
            Ts.append((R, t))
            zs.append(c.z[a])
            ws.append(c.weight[a])
        x4 = c.x_w[l]
        if LM == 1:
            p = Rsr @ x4[:3] + tsr * x4[3]
            ray, rho = p / np.linalg.norm(p), x4[3] / np.linalg.norm(p)
            first_c, first_d = np.zeros(3), ray
        else:
            X, rho = x4[:3].copy(), x4[3]
            first_c, first_d = -Ts[0][0].T @ Ts[0][1], Ts[0][0].T @ bearing(cams[0], zs[0])
        cen = [-R.T @ t for R, t in Ts]
        dirs = [R.T @ bearing(cm, z) for (R, t), cm, z in zip(Ts, cams, zs)]
        with np.errstate(all="ignore"):
            parallax = max(_angle(first_d, d) for d in dirs)
            base2 = max(float((cc - first_c) @ (cc - first_c)) for cc in cen)
            if o["linear_init"]:
                if LM == 3:
                    A, q = np.zeros((3, 3)), np.zeros(3)
                    for w, cc, d in zip(ws, cen, dirs):
                        M = w * (np.eye(3) - np.outer(d, d))
                        A += M
                        q += M @ cc
                    try:
                        X = np.linalg.solve(A, q)
                    except np.linalg.LinAlgError:
                        X = np.full(3, np.nan)
                    rho = 1.0
                else:
                    num = den = 0.0
                    for w, (R, t), cm, z in zip(ws, Ts, cams, zs):
                        b = bearing(cm, z)
                        br, bt = np.cross(b, R @ ray), np.cross(b, t)
                        num += w * (br @ bt)
                        den += w * (bt @ bt)
                    rho = -num / den

            def sums(x, guard):
                V, bl, E, dmin = np.zeros((LM, LM)), np.zeros(LM), 0.0, np.inf
                for w0, (R, t), cm, z in zip(ws, Ts, cams, zs):
                    P = R @ x + t * rho if LM == 3 else R @ ray * 1.0 + t * x[0]
                    uv, dpi = project(cm, P)
                    r = z - uv
                    J = -dpi @ R if LM == 3 else -(dpi @ t).reshape(2, 1)
                    w = w0
                    if o["huber_width"] > 0:
                        en = np.sqrt((r @ r) * w)
                        if en > o["huber_width"]:
                            w *= o["huber_width"] / en
                    V += w * J.T @ J
                    bl += w * J.T @ r
                    dep = P[2]
                    E += w * (r @ r) if not (guard and not dep > 0) else np.inf
                    dmin = min(dmin, dep) if not np.isnan(dep) else np.nan
                return V, bl, E, dmin

            x = X.copy() if LM == 3 else np.array([rho])
            V, bl, E, depth = sums(x, False)
            res[l] = [TOO_FEW_VIEWS, k, 0, E, E, parallax, depth, 0]
            if k < 2 or base2 <= BASELINE_REL ** 2 * (1.0 + first_c @ first_c):
                continue
            if not (np.all(np.isfinite(x)) and np.isfinite(E) and np.isfinite(depth)):
                res[l, 0] = FAILED
                continue
            if parallax < o["min_parallax"]:
                res[l, 0] = LOW_PARALLAX
                continue
            if depth <= 0:
                res[l, 0] = BEHIND_CAMERA
                continue
            lam, nu, it, E0 = o["lambda0"], 2.0, 0, E
            while True:
                cg = 0.0 if E == 0 else max(abs(bl[i]) / np.sqrt(V[i, i] * E) for i in range(LM))
                if E == 0 or cg <= o["gradient_tolerance"]:
                    status = OK
                    break
                if it >= o["max_iterations"]:
                    status = NOT_CONVERGED
                    break
                D = np.diag([_clamp(V[i, i]) for i in range(LM)])
                try:
                    delta = np.linalg.solve(V + lam * D, bl)
                except np.linalg.LinAlgError:
                    delta = np.full(LM, np.nan)
                pred = delta @ (lam * D @ delta + bl)
                Vt, bt_, Et, _ = sums(x - delta, True)
                gain = (E - Et) / pred
                lam, nu, accept = _nielsen(lam, nu, gain)
                it += 1
                if accept:
                    x, V, bl, E = x - delta, Vt, bt_, Et
                    if o["step_tolerance"] > 0 and np.linalg.norm(delta) <= o["step_tolerance"] * (np.linalg.norm(x) + o["step_tolerance"]):
                        cg = 0.0 if E == 0 else max(abs(bl[i]) / np.sqrt(V[i, i] * E) for i in range(LM))
                        status = OK
                        break
            _, _, _, depth = sums(x, False)
            res[l] = [status, k, it, E0, E, parallax, depth, cg]
            final[l] = (V.copy(), lam, np.diag([_clamp(V[i, i]) for i in range(LM)]), x.copy(), it)
            if status == OK or (E <= E0 if o["linear_init"] else E < E0):
                if LM == 3:
                    xw[l] = np.append(x, rho)
                else:
                    xw[l] = np.append(Rwr @ ray + twr * x[0], x[0])
    return res, xw, final


def params(c, xw):
    """the landmark's own parameters out of world coordinates: the point (LmSize 3), the inverse depth (LmSize 1)"""
    return xw[:, :3] if c.lm_dim == 3 else xw[:, 3:4]


def coordinate_bound(c, final, l, step_tolerance):
    """2 step_tolerance |x| + 8 cond2(V + lambda D) eps |x| of landmark l, from the restatement's end point"""
    V, lam, D, x, _ = final[l]
    nx = np.linalg.norm(x)
    return 2.0 * step_tolerance * nx + 8.0 * np.linalg.cond(V + lam * D) * EPS * nx


def linear_condition(c, l):
    """cond2 of the linear estimate's matrix sum w (I - d d^T) of landmark l (LmSize 3), and its smallest... parallax"""
    tws, tsw = tables(c)
    A = np.zeros((3, 3))
    for a in np.nonzero(c.lm == l)[0]:
        R, t = tsw[c.pose[a]][c.cam[a]]
        ip = c.cam_params[c.cam[a]]
        d = R.T @ bearing((ip[0], ip[1], ip[2], ip[3], c.cam_w[c.cam[a]], int(c.cam_model[c.cam[a]])), c.z[a])
        A += c.weight[a] * (np.eye(3) - np.outer(d, d))
    return np.linalg.cond(A)


# ---- the host restatement (ba_hostcheck_triangulate) ----------------------------------------------------------------
def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def sorted_tables(c):
    """the observations sorted by landmark (stable) with the CSR over them"""
    order = np.argsort(c.lm, kind="stable")
    ptr = np.zeros(len(c.x_w) + 1, dtype=np.uint32)
    np.cumsum(np.bincount(c.lm, minlength=len(c.x_w)), out=ptr[1:])
    return order, ptr


def triangulate_host(hc, c, opts=None, ids=None):
    """-> (res [L, 8], x_w [L, 4], final [L, 10]) or the message of the refusal"""
    o = options(**(opts or {}))
    order, ptr = sorted_tables(c)
    L = len(c.x_w)
    f64, u32 = np.float64, np.uint32
    con = lambda a, t: np.ascontiguousarray(a, dtype=t)
    pose, cam, z, w = con(c.pose[order], u32), con(c.cam[order], u32), con(c.z[order], f64), con(c.weight[order], f64)
    opts8 = np.array([o[k] for k in ("linear_init", "max_iterations", "write_back", "lambda0", "gradient_tolerance",
                                     "step_tolerance", "min_parallax", "huber_width")], dtype=f64)
    res, xw, final = np.zeros((L, 8)), np.zeros((L, 4)), np.zeros((L, 10))
    ida = None if ids is None else con(ids, u32)
    msg = ctypes.create_string_buffer(512)
    dbl, U32 = ctypes.c_double, ctypes.c_uint32
    poses = con(c.poses[:, :7], f64)
    pose_cam = None if c.pose_cam is None else con(c.pose_cam, f64)
    hc.ba_hostcheck_triangulate.restype = ctypes.c_int
    rc = hc.ba_hostcheck_triangulate(
        c.lm_dim, U32(len(poses)), _ptr(poses, dbl), U32(len(c.cam_params)), _ptr(con(c.cam_params, f64), dbl),
        _ptr(con(c.cam_tvs, f64), dbl), _ptr(con(c.cam_model, np.int32), ctypes.c_int32), _ptr(con(c.cam_w, f64), dbl),
        _ptr(pose_cam, dbl), U32(L), _ptr(ptr, U32), _ptr(pose, U32), _ptr(cam, U32), _ptr(z, dbl), _ptr(w, dbl),
        _ptr(con(c.x_w, f64), dbl), _ptr(con(c.ref_pose, u32), U32), _ptr(con(c.ref_cam, u32), U32), None,
        U32(0 if ida is None else len(ida)), _ptr(ida, U32), _ptr(opts8, dbl), _ptr(res, dbl), _ptr(xw, dbl), _ptr(final, dbl),
        msg, U32(512))
    assert rc in (0, 1), rc
    if rc:
        return msg.value.decode()
    return res, xw, final


# ---- on the device ------------------------------------------------------------------------------------------------
def engine(c, robust=False, finalize=True):
    """a hipapi.Engine on the case, finalized"""
    from ba_amd import hipapi
    eng = hipapi.Engine(c.lm_dim, 6)
    o = hipapi.Options()
    o.projection_outlier_threshold = 1.0
    o.use_robust_norm_for_proj_residuals = 1 if robust else 0
    eng.set_options(o)
    eng.set_cameras(c.cam_params, c.cam_tvs)
    if c.cam_model.any():
        eng.set_camera_models(c.cam_model, c.cam_w)
    pa = np.ones(len(c.poses), dtype=np.uint8)
    pa[0] = 0
    eng.set_poses(c.poses, is_active=pa)
    eng.set_landmarks(c.x_w, c.ref_pose, ref_cam=c.ref_cam, is_active=c.lm_active)
    eng.set_projection_residuals(c.z, c.pose, c.lm, cam=c.cam, weight=c.weight)
    if c.pose_cam is not None:
        eng.set_pose_cam_params(c.pose_cam)
    if finalize:
        eng.finalize()
    return eng
