"""The step path -- everything between the reduced solve and the next linearisation -- on graphs that put inactive,
unobserved and lone landmarks on the edges of the 256-thread blocks: the cases, a long-double reference computed from
per-residual inputs, a plain float64 numpy restatement (with switchable mistakes) and ONE comparator.  Shared by
test_step_path.py (CPU: the oracle's outputs and the restatement stay inside every bound, every mistake is caught) and
test_step_path_gpu.py (the engine's taps through the same comparator).  numpy only.

Code under test: k_backsub<1|3> with its calibration term, k_dots_pose / k_dots_lm / k_jrhs / k_jk_rhs /
launch_calib_dogleg, the reused steepest-descent denominator, k_compose / k_compose_lm, k_sum_partials(_l1) with the
deferred flush, k_apply_poses / k_apply_landmarks<1|3> / ba_hip_rollback and k_sensor_to_world.

A "bundle" is a namespace the comparator reads; a part that is absent is not compared:

    case                          the case (below)
    lin                           jm, jr, jl (2 x 6, 2 x 6, 2 x LM), r (2), jk (2 x 6, K = 6 only) per accepted residual id,
                                  all weighted by sqrt(w); masked columns zero
    rhs_p, gn_p                   n + K entries, active poses in id order, the calibration tail behind them
    rhs_l, gn_l                   by optimisation index (active landmarks in id order)
    system                        False: gn_p / gn_l do not belong to `lin`, the full-system figures are left out
    scal0, scal1                  the ten dogleg scalars without / with the Gauss-Newton step (dicts)
    pp_jrhs, pp_tol               the pose-pose part of j_rhs_sq from elsewhere and what it is known to (vi15)
    steps                         [namespace(a, b, step_p, step_l, norm_p, norm_l)]
    updates                       [namespace(step_p, step_l, before, after)], a state = namespace(poses P x 7, vel P x 3,
                                  bias P x 6, lms L x 4 (LmSize 3) or None, rho L (LmSize 1; `after` may lack it), rel L)
    world                         namespace(x_w0, poses0, t_vs0, poses1, t_vs1, rho1, x_w1, rho0): LmSize 1 after end_solve

Bounds.  eps = 2^-52.
  * full system: H = J^T J over active pose, calibration and landmark columns, masked columns zero with 1e6 on the
    diagonal, the V guard of BundleAdjuster.cpp:431-439, g = J^T r; max_i |H d - g|_i / (|H| |d| + |g|)_i in eps.  No
    fixed bound: 8 x what the oracle's own step reaches on the same case (a different elimination order is allowed
    for; a wrong incidence moves the figure by more than 1e5).
  * sums: |got - long-double sum| <= c eps sum |term|, c the longest chain of additions plus the roundings of a
    term, counted in chain() and the functions that use it.
  * composed step: 2 eps (|a rhs| + |b gn|) per entry; bitwise a * rhs when b == 0.
  * update: bitwise x - d; rotation normalise(q (x) exp(-d)) within 16 eps per component (quaternion product: 4
    products and 3 additions per component, the normalisation 3 more roundings, exp another 4, on unit quaternions).
  * world coordinates: 64 eps (|x| + |t_ref|) per coordinate."""
import types

import numpy as np

from ba_amd import scene

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
MASK_DIAGONAL = 1e6
V_GUARD = 1e-6
SMALL_ANGLE = 1e-10                       # so3_exp: the series below, sin / cos above (dmath.h)
ROTATION_BOUND, RESTATEMENT_ROTATION_BOUND = 16.0, 4.0
WORLD_BOUND = 64.0
SYSTEM_FACTOR = 8.0
ROTATION_LADDER = (0.0, 1e-12, 1e-9, 1e-3, 3.0, 6.0)     # largest rotation step of a rung, rad
T_VS_MOUNT = np.concatenate([[0.05, -0.02, 0.1], scene.quat_exp(np.array([0.02, -0.03, 0.01]))])
TVS_PERTURB = np.array([0.06, -0.05, 0.05, 0.02, -0.03, 0.02])
IDENTITY_T = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
SCALARS = ("rhs_p_sq", "rhs_l_sq", "j_rhs_sq", "gn_p_sq", "gn_l_sq", "rhs_gn_p", "rhs_gn_l", "rhs_k_sq", "gn_k_sq",
           "rhs_gn_k")
L1_THRESHOLD = 8192                       # sum_partials: more partials than this take k_sum_partials_l1 first


# ---- cases ----------------------------------------------------------------------------------------------------
NO_RESIDUAL, TWICE_SEEN, REGULARISED_POSE = 100, 200, 10
EDGE_INACTIVE_POSES = (0, 24, 1, 25)      # the two anchors of make_scene(48, ...) and their neighbours


def opt_ids(active):
    o = np.full(len(active), -1, dtype=np.int64)
    o[np.asarray(active) > 0] = np.arange(int(np.asarray(active).sum()))
    return o


def _finish(name, LM, D, sc, pa, la, masks, table, K=0, t_vs=IDENTITY_T, regularize=(), imu=False):
    z, pose, lm = table
    acc = np.ones(len(pose), dtype=bool) if LM != 1 else pose != sc.lm_ref_pose[lm]
    c = types.SimpleNamespace(
        name=name, LM=LM, D=D, K=K, sc=sc, pa=np.asarray(pa, np.uint8), la=np.asarray(la, np.uint8),
        masks=np.asarray(masks, np.uint16), obs_z=np.ascontiguousarray(z), obs_pose=pose.astype(np.uint32),
        obs_lm=lm.astype(np.uint32), z=np.ascontiguousarray(z[acc]), pose=pose[acc].astype(np.uint32),
        lm=lm[acc].astype(np.uint32), t_vs=np.asarray(t_vs, np.float64), regularize=tuple(regularize), imu=imu)
    c.P, c.L, c.O = sc.num_poses, sc.num_landmarks, int(acc.sum())
    c.n, c.nl = int(c.pa.sum()) * D, int(c.la.sum()) * LM
    c.ref = sc.lm_ref_pose[c.lm].astype(np.int64)
    return c


def edges(lm_dim, inactive_landmarks=(0, 255), name=None):
    """48 poses, 4 inactive (n = 264: two blocks of pose entries, 8 in the second); 257 landmarks with 1285 accepted
    residuals (six blocks, 5 in the last); landmarks 0 and 255 inactive, 256 alone in the second block (inactive with
    LmSize 3); landmark 100 active without an accepted residual (LmSize 1: seen from its reference pose only), its
    five observations given to landmark 200 (seen twice from each pose); one active landmark measured from inactive
    poses only; pose 10 with its translation regularised.  Residual ids are shuffled."""
    P, L, k = 48, 257, 5
    sc = scene.make_scene(P, L, k, lm_dim=lm_dim, seed=7)
    nsel = k + (1 if lm_dim == 1 else 0)
    first = nsel - k
    inactive = np.array(EDGE_INACTIVE_POSES)
    assert set(sc.anchor_poses.tolist()) <= set(inactive.tolist())
    pa = np.ones(P, np.uint8)
    pa[inactive] = 0
    la = np.ones(L, np.uint8)
    la[list(inactive_landmarks)] = 0
    if lm_dim == 3:
        la[256] = 0
    zt, pt = sc.obs_z.reshape(L, nsel, 2).copy(), sc.obs_pose.reshape(L, nsel).copy()
    rng = np.random.Generator(np.random.PCG64([7, 0x57E9, lm_dim]))
    only_inactive = None
    for l in range(1, 254):
        if l in (NO_RESIDUAL, TWICE_SEEN) or (lm_dim == 1 and not pa[sc.lm_ref_pose[l]]):
            continue
        uv, depth = scene.project(sc.gt_poses[inactive], np.broadcast_to(sc.gt_landmarks[l, :3], (len(inactive), 3)))
        vis = (depth > 0.5) & (uv[:, 0] > 0) & (uv[:, 0] < scene.IMG_W) & (uv[:, 1] > 0) & (uv[:, 1] < scene.IMG_H)
        if vis.sum() >= 2:
            pick = np.nonzero(vis)[0][np.arange(k) % int(vis.sum())]
            pt[l, first:] = inactive[pick]
            zt[l, first:] = uv[pick] + rng.normal(0.0, 1.5, (k, 2))
            only_inactive = l
            break
    assert only_inactive is not None
    zs, ps, ls = [], [], []
    for l in range(L):
        keep = first if l == NO_RESIDUAL else nsel
        zs.append(zt[l, :keep])
        ps.append(pt[l, :keep])
        if l == TWICE_SEEN:
            zs.append(zt[l, first:] + rng.normal(0.0, 0.3, (k, 2)))
            ps.append(pt[l, first:])
        ls.append(np.full(sum(len(x) for x in ps) - sum(len(x) for x in ls), l))
    z, pose, lm = np.concatenate(zs), np.concatenate(ps), np.concatenate(ls)
    perm = np.random.Generator(np.random.PCG64([7, 0x57E9, 99])).permutation(len(pose))
    masks = np.zeros(P, np.uint16)
    masks[REGULARISED_POSE] = 0x7
    c = _finish(name or "edges_lm%d" % lm_dim, lm_dim, 6, sc, pa, la, masks, (z[perm], pose[perm], lm[perm]),
                regularize=[(REGULARISED_POSE, 1, 0, 0, 0)])
    c.only_inactive, c.no_residual, c.twice_seen = only_inactive, NO_RESIDUAL, TWICE_SEEN
    return c


def edges_lm1_last_active():
    """edges_lm1 with landmark 254 inactive in place of 255: the last landmark of the first block counts.  (With 255
    inactive, as the other cases have it, a sum that loses thread 255 of a block loses nothing.)"""
    return edges(1, inactive_landmarks=(0, 254), name="edges_lm1_last_active")


def exp_decoupled(t7, x6):
    """t + x[:3], q (x) exp(x[3:]) in float64 (Utils.h:364-369)"""
    q = scene.quat_mul(np.asarray(t7[3:7]), scene.quat_exp(np.asarray(x6[3:6])))
    return np.concatenate([np.asarray(t7[:3]) + np.asarray(x6[:3]), q / np.linalg.norm(q)])


def tvs():
    """LmSize 1 with the camera mount as six calibration unknowns (K = 6): 30 poses on the banked trajectory, every
    third one held at ground truth, 60 landmarks handed over for a wrong mount guess (tests/test_gpu_parity.py:
    _calib_scene)."""
    P, L, k = 30, 60, 6
    sc = scene.mount_camera(scene.make_scene(P, L, k, lm_dim=1, seed=7, roll_amp=0.6), T_VS_MOUNT)
    pa = np.ones(P, np.uint8)
    pa[::3] = 0
    sc.poses[::3] = sc.gt_poses[::3]
    t0 = exp_decoupled(T_VS_MOUNT, TVS_PERTURB)
    sc.landmarks = scene.remount_landmarks(sc, T_VS_MOUNT, t0)
    return _finish("tvs", 1, 6, sc, pa, np.ones(L, np.uint8), np.zeros(P, np.uint16), (sc.obs_z, sc.obs_pose, sc.obs_lm),
                   K=6, t_vs=t0)


VI_MASK = 0x37 | 0x7E00    # RegularizePose(translation, bias, rotation): parameters 0 1 2 | 2 4 5 | 9 .. 14


def vi15():
    """LmSize 1, PoseSize 15: 18 poses, all active (n = 270), an inertial residual per neighbour pair, 70 landmarks;
    pose 0 regularised (position, yaw and pitch, biases) in place of the automatic regularisation."""
    P, L, k = 18, 70, 5
    sc = scene.make_scene(P, L, k, lm_dim=1, seed=51)
    scene.add_inertial(sc, period=60.0 * P / 100.0)
    masks = np.zeros(P, np.uint16)
    masks[0] = VI_MASK
    return _finish("vi15", 1, 15, sc, np.ones(P, np.uint8), np.ones(L, np.uint8), masks,
                   (sc.obs_z, sc.obs_pose, sc.obs_lm), regularize=[(0, 1, 0, 1, 1)], imu=True)


LONG_TRACK = 33            # two such landmarks do not fit one 64-observation range: one partial per landmark


def long_sums(n_landmarks):
    """LmSize 1, `n_landmarks` landmarks of 33 accepted residuals each (every landmark of make_scene(40, ., 5) seen
    again and again from its five poses, 0.5 px apart): ba_hip_linearize sums one partial per landmark."""
    sc = scene.make_scene(40, n_landmarks, 5, lm_dim=1, seed=3)
    L = n_landmarks
    zt, pt = sc.obs_z.reshape(L, 6, 2)[:, 1:], sc.obs_pose.reshape(L, 6)[:, 1:]
    idx = np.arange(LONG_TRACK) % 5
    rng = np.random.Generator(np.random.PCG64([3, 0x57E9, 33]))
    z = zt[:, idx] + rng.normal(0.0, 0.5, (L, LONG_TRACK, 2))
    pa = np.ones(40, np.uint8)
    pa[sc.anchor_poses] = 0
    return _finish("long_sums_%d" % L, 1, 6, sc, pa, np.ones(L, np.uint8), np.zeros(40, np.uint16),
                   (z.reshape(-1, 2), pt[:, idx].reshape(-1), np.repeat(np.arange(L), LONG_TRACK)))


CASES = {"edges_lm1": lambda: edges(1), "edges_lm3": lambda: edges(3), "edges_lm1_last_active": edges_lm1_last_active,
         "vi15": vi15, "tvs": tvs}
_cases = {}


def case(name):
    """one case per name and process; read only"""
    if name not in _cases:
        _cases[name] = CASES[name]()
    return _cases[name]


def initial_state(c):
    """the state a Solve starts from, as float64 arrays (rho of LmSize 1 left to the caller: it is a device result)"""
    sc = c.sc
    vel = np.array(getattr(sc, "init_vel", np.zeros((c.P, 3))), dtype=np.float64)
    bias = np.array(getattr(sc, "init_bias", np.zeros((c.P, 6))), dtype=np.float64)
    return types.SimpleNamespace(poses=sc.poses.copy(), vel=vel, bias=bias, lms=sc.landmarks.copy() if c.LM == 3 else None,
                                 rho=None, rel=np.ones(c.L, np.uint8))


# ---- per-residual columns and Jacobians -----------------------------------------------------------------------
def columns(c):
    """(O, 12 + K + LM) column of every local Jacobian entry in [poses | calibration | landmarks]; the column
    n + K + nl collects what belongs to inactive poses and landmarks (and the reference side of LmSize 3)"""
    popt, lopt = opt_ids(c.pa), opt_ids(c.la)
    trash = c.n + c.K + c.nl
    idx = np.full((c.O, 12 + c.K + c.LM), trash, dtype=np.int64)
    six = np.arange(6)
    m = popt[c.pose]
    idx[:, :6] = np.where(m[:, None] >= 0, m[:, None] * c.D + six, trash)
    if c.LM == 1:
        r = popt[c.ref]
        idx[:, 6:12] = np.where(r[:, None] >= 0, r[:, None] * c.D + six, trash)
    idx[:, 12:12 + c.K] = c.n + np.arange(c.K)
    lo = lopt[c.lm]
    idx[:, 12 + c.K:] = np.where(lo[:, None] >= 0, c.n + c.K + lo[:, None] * c.LM + np.arange(c.LM), trash)
    return idx


def local_jacobian(c, lin, dtype=LD):
    """(O, 2, 12 + K + LM): [jm | jr | jk | jl] with the masked pose columns zero"""
    J = np.zeros((c.O, 2, 12 + c.K + c.LM), dtype=dtype)
    bits = (c.masks[:, None].astype(np.int64) >> np.arange(6)) & 1
    J[:, :, :6] = np.asarray(lin.jm, dtype=dtype) * (1 - bits[c.pose])[:, None, :]
    if c.LM == 1:
        J[:, :, 6:12] = np.asarray(lin.jr, dtype=dtype) * (1 - bits[c.ref])[:, None, :]
    if c.K:
        J[:, :, 12:12 + c.K] = np.asarray(lin.jk, dtype=dtype)
    J[:, :, 12 + c.K:] = np.asarray(lin.jl, dtype=dtype)
    return J


def masked_rows(c):
    popt = opt_ids(c.pa)
    return [popt[p] * c.D + k for p in range(c.P) if popt[p] >= 0 for k in range(c.D) if (int(c.masks[p]) >> k) & 1]


def _guard(H, c):
    o = c.n + c.K
    for q in range(c.nl // c.LM if c.LM else 0):
        s = slice(o + q * c.LM, o + (q + 1) * c.LM)
        blk = H[s, s]
        if c.LM == 1:
            if abs(blk[0, 0]) < V_GUARD:
                blk[0, 0] += V_GUARD
        elif np.sqrt((blk * blk).sum()) < V_GUARD:
            blk[np.arange(3), np.arange(3)] += V_GUARD


def full_system(c, lin):
    """(H, g) in long double; computed once per set of Jacobians"""
    if getattr(lin, "_system", None) is None:
        idx, J = columns(c), local_jacobian(c, lin)
        N = c.n + c.K + c.nl
        H, g = np.zeros((N + 1, N + 1), dtype=LD), np.zeros(N + 1, dtype=LD)
        np.add.at(H, (idx[:, :, None], idx[:, None, :]), np.einsum("ori,orj->oij", J, J))
        np.add.at(g, idx, np.einsum("ori,or->oi", J, np.asarray(lin.r, dtype=LD)))
        H, g = H[:N, :N].copy(), g[:N].copy()
        for i in masked_rows(c):
            H[i, :] = 0
            H[:, i] = 0
            H[i, i] = MASK_DIAGONAL
            g[i] = 0
        _guard(H, c)
        lin._system = (H, g)
    return lin._system


def system_ratios(c, lin, dp, dl):
    """max_i |H d - g|_i / (|H| |d| + |g|)_i in eps over the landmark rows and over the pose rows -> ((value, row), ...)"""
    H, g = full_system(c, lin)
    d = np.concatenate([np.asarray(dp, dtype=LD), np.asarray(dl, dtype=LD)])
    res, den = np.abs(H @ d - g), np.abs(H) @ np.abs(d) + np.abs(g)
    ratio = np.where(den > 0, res / np.where(den > 0, den, 1), np.where(res > 0, np.inf, 0.0)) / EPS
    ratio = np.where(np.isfinite(np.asarray(d, dtype=np.float64)).all(), ratio, np.inf)
    o = c.n + c.K
    lm = (float(ratio[o:].max()), int(ratio[o:].argmax())) if c.nl else (0.0, -1)
    return lm, (float(ratio[:c.n].max()), int(ratio[:c.n].argmax()))


# ---- sums -----------------------------------------------------------------------------------------------------
TREE = 8                                   # levels of the 256-thread shared-memory tree


def chain(nparts):
    """additions a term passes through from its thread to the result: the tree of its block, then k_sum_partials (a
    strided pass of ceil(nparts / 256) additions and a tree); more than 8192 partials go through k_sum_partials_l1
    first (64 blocks: a strided pass over ceil(nparts / 64) entries, a tree), which leaves 64 for k_sum_partials"""
    if nparts > L1_THRESHOLD:
        return TREE + (-(-(-(-nparts // 64)) // 256) + TREE) + (1 + TREE)
    return TREE + -(-max(nparts, 1) // 256) + TREE


def _blocks(n):
    return -(-n // 256)


def chain_counts(c, shards=1):
    """c of |got - sum| <= c eps sum |term| per dogleg scalar (and the step norms), from the kernels:
      pose dots     one product, chain(blocks of n)
      landmark dots one product and LM additions in the thread, chain(blocks of L), one addition across shards
      calibration   six products and additions on the host
      j_rhs_sq      v = sum of 12 + LM products (13 + LM roundings against sum |J g|), v^2 doubles that and adds one,
                    v0^2 + v1^2 one more, chain(blocks of O), the sum across shards, three additions of the parts
                    (pose-pose, priors, calibration)
    Every count is below 64."""
    pose = 1 + chain(_blocks(c.n))
    lm = 1 + c.LM + chain(_blocks(c.L)) + (shards > 1)
    jr = 2 * (13 + c.LM) + 2 + chain(_blocks(c.O)) + (shards > 1) + 3
    out = dict(rhs_p_sq=pose, gn_p_sq=pose, rhs_gn_p=pose, rhs_l_sq=lm, gn_l_sq=lm, rhs_gn_l=lm, j_rhs_sq=jr,
               rhs_k_sq=7, gn_k_sq=7, rhs_gn_k=7, norm_p=pose + 3, norm_l=lm + 3)   # (+ 3: the square root, squared again)
    assert max(out.values()) < 64
    return out


def dogleg_reference(c, lin, rhs_p, rhs_l, gn_p, gn_l, gn_ok):
    """name -> (long-double sum, sum of the magnitudes of its terms)"""
    f = lambda v: np.asarray(v, dtype=LD)
    rp, rk, gp, gk = f(rhs_p[:c.n]), f(rhs_p[c.n:]), f(gn_p[:c.n]) * gn_ok, f(gn_p[c.n:]) * gn_ok
    rl, gl = f(rhs_l), f(gn_l) * gn_ok
    if not gn_ok:
        gp, gk, gl = np.zeros_like(rp), np.zeros_like(rk), np.zeros_like(rl)
    out = {}
    for tag, r, g in (("p", rp, gp), ("l", rl, gl), ("k", rk, gk)):
        out["rhs_%s_sq" % tag] = ((r * r).sum(), (r * r).sum())
        out["gn_%s_sq" % tag] = ((g * g).sum(), (g * g).sum())
        out["rhs_gn_%s" % tag] = ((r * g).sum(), np.abs(r * g).sum())
    # |J rhs|^2: per residual v = Jm g_m + Jr g_r + Jl g_l, and u = Jk g_k as a term of its own (BundleAdjuster.cpp:881-910)
    grad = np.concatenate([f(rhs_p), rl, np.zeros(1, dtype=LD)])
    T = local_jacobian(c, lin) * grad[columns(c)][:, None, :]
    cal = np.zeros(T.shape[2], dtype=bool)
    cal[12:12 + c.K] = True
    v, u = T[:, :, ~cal].sum(2), T[:, :, cal].sum(2)
    sv, su = np.abs(T[:, :, ~cal]).sum(2), np.abs(T[:, :, cal]).sum(2)
    out["j_rhs_sq"] = ((v * v).sum() + (u * u).sum(), (sv * sv).sum() + (su * su).sum())
    return out


# ---- rotations in long double ---------------------------------------------------------------------------------
def quat_mul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def so3_exp(w):
    """unit quaternion of the rotation vector w: the closed form (what the series below 1e-10 expands)"""
    w = np.asarray(w)
    th = np.sqrt((w * w).sum(-1, keepdims=True))
    safe = np.where(th > 0, th, 1)
    imag = np.where(th > 0, np.sin(th / 2) / safe, w.dtype.type(0.5))
    return np.concatenate([imag * w, np.cos(th / 2)], -1)


def so3_exp_float64(w, sin_theta=False):
    """so3_exp of dmath.h, restated: both branches, then normalised"""
    w = np.asarray(w, dtype=np.float64)
    th2 = (w * w).sum(-1, keepdims=True)
    th = np.sqrt(th2)
    small = th < SMALL_ANGLE
    safe = np.where(small, 1.0, th)
    imag = np.where(small, 0.5 - th2 / 48.0 + th2 * th2 / 3840.0, np.sin(th if sin_theta else 0.5 * th) / safe)
    real = np.where(small, 1.0 - th2 / 8.0 + th2 * th2 / 384.0, np.cos(0.5 * th))
    q = np.concatenate([imag * w, real], -1)
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def quat_to_rot(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3), dtype=q.dtype)
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def _unit(q):
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def sensor_frames(poses, t_vs, dtype=LD):
    """(R_ws, t_ws) of T_ws = T_wp T_vs per pose"""
    p, v = np.asarray(poses, dtype=dtype), np.asarray(t_vs, dtype=dtype)
    Rp = quat_to_rot(_unit(p[:, 3:7]))
    return Rp @ quat_to_rot(_unit(v[3:7])), Rp @ v[:3] + p[:, :3]


def world_to_sensor(c, x_w, poses, t_vs, dtype=LD):
    """(x_s unit rays L x 3, rho L) of k_world_to_sensor"""
    R, t = sensor_frames(poses, t_vs, dtype)
    ref = c.sc.lm_ref_pose.astype(np.int64)
    x = np.asarray(x_w, dtype=dtype)
    p = np.einsum("lji,lj->li", R[ref], x[:, :3] - t[ref] * x[:, 3:4])
    ln = np.sqrt((p * p).sum(-1))
    return p / ln[:, None], x[:, 3] / ln, ln


def sensor_to_world(c, x_s, rho, poses, t_vs, dtype=LD):
    R, t = sensor_frames(poses, t_vs, dtype)
    ref = c.sc.lm_ref_pose.astype(np.int64)
    return np.einsum("lij,lj->li", R[ref], np.asarray(x_s, dtype=dtype)) + t[ref] * np.asarray(rho, dtype=dtype)[:, None], t[ref]


# ---- the comparator -------------------------------------------------------------------------------------------
def _fig(figs, name, value, bound, where=None):
    figs[name] = types.SimpleNamespace(value=float(value), bound=float(bound), where=where)


def _worst(err, tol):
    """(max err / tol, its index) with 0 / 0 = 0 and x / 0 = inf"""
    err, tol = np.asarray(err, dtype=LD).ravel(), np.asarray(tol, dtype=LD).ravel()
    if err.size == 0:
        return 0.0, -1
    err = np.where(np.isfinite(err.astype(np.float64)), err, np.inf)
    q = np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0.0))
    return float(q.max()), int(q.argmax())


def _bits(figs, name, a, b):
    n, i = _mismatches(a, b)
    _fig(figs, name, n, 0, i)


def _mismatches(a, b):
    """entries that differ in their bits (-0.0 == 0.0 and NaN != NaN, as the float comparison has it) -> (count, first)"""
    bad = np.nonzero(~(np.asarray(a) == np.asarray(b)).ravel())[0]
    return len(bad), (int(bad[0]) if len(bad) else -1)


def compare_scalars(figs, tag, c, got, ref, counts, pp_jrhs=0.0, pp_tol=0.0):
    for k in SCALARS:
        val, scale = ref[k]
        tol = counts[k] * EPS * scale
        if k == "j_rhs_sq":
            val, tol = val + LD(pp_jrhs), tol + LD(pp_tol)
        e, _ = _worst([abs(LD(got[k]) - val)], [tol])
        _fig(figs, "%s.%s" % (tag, k), e, 1.0, "%.17g against %.17g, c = %d" % (got[k], float(val), counts[k]))


def compare_step(figs, tag, c, s, rhs_p, rhs_l, gn_p, gn_l, counts):
    a, b = LD(s.a), LD(s.b)
    f = lambda v: np.asarray(v, dtype=LD)
    for part, got, r, g in (("p", s.step_p[:c.n], rhs_p[:c.n], gn_p[:c.n]), ("k_tail", s.step_p[c.n:], rhs_p[c.n:], gn_p[c.n:]),
                            ("l", s.step_l, rhs_l, gn_l)):
        if s.b == 0.0:
            n, i = _mismatches(got, s.a * np.asarray(r))
            _fig(figs, "%s.%s_bitwise" % (tag, part), n, 0, i)
        else:
            want, tol = a * f(r) + b * f(g), 2 * EPS * (np.abs(a * f(r)) + np.abs(b * f(g)))
            e, i = _worst(np.abs(f(got) - want), tol)
            _fig(figs, "%s.%s" % (tag, part), e, 1.0, i)
    for part, got, norm in (("norm_p", s.step_p[:c.n], s.norm_p), ("norm_l", s.step_l, s.norm_l)):
        sq = (f(got) ** 2).sum()
        e, _ = _worst([abs(LD(norm) * LD(norm) - sq)], [counts[part] * EPS * sq])
        _fig(figs, "%s.%s" % (tag, part), e, 1.0, "%.17g against %.17g" % (norm, float(np.sqrt(sq))))


def update_reference(c, before, step_p, step_l):
    """what ApplyUpdate makes of `before` (BundleAdjuster.cpp:84-139): float64 arrays for what has to be bitwise, the
    rotations in long double"""
    popt, lopt = opt_ids(c.pa), opt_ids(c.la)
    act = np.nonzero(popt >= 0)[0]
    d = np.asarray(step_p[:c.n], dtype=np.float64).reshape(-1, c.D)[popt[act]]
    w = types.SimpleNamespace(poses=before.poses.copy(), vel=before.vel.copy(), bias=before.bias.copy(), act=act,
                              lms=None, rho=None, rel=before.rel.copy())
    w.poses[act, :3] = before.poses[act, :3] - d[:, :3]
    q = np.asarray(before.poses[:, 3:7], dtype=LD)
    q[act] = _unit(quat_mul(q[act], so3_exp(-np.asarray(d[:, 3:6], dtype=LD))))
    w.quat = q
    if c.D >= 9:
        w.vel[act] = before.vel[act] - d[:, 6:9]
    if c.D >= 15:
        w.bias[act] = before.bias[act] - d[:, 9:15]
    la = np.nonzero(lopt >= 0)[0]
    dl = np.asarray(step_l, dtype=np.float64).reshape(-1, max(c.LM, 1))[lopt[la]]
    if c.LM == 3:
        w.lms = before.lms.copy()
        w.lms[la, :3] = before.lms[la, :3] - dl
    elif c.LM == 1 and before.rho is not None:
        w.rho = before.rho.copy()
        moved = before.rho[la] - dl[:, 0]
        neg = moved < 0
        w.rho[la] = np.where(neg, moved + dl[:, 0], moved)       # BundleAdjuster.cpp:128-132: put back by adding again
        w.rel[la[neg]] = 0
        w.negative = la[neg]
    return w


def compare_update(figs, tag, c, u):
    w = update_reference(c, u.before, u.step_p, u.step_l)
    a = u.after
    inact = np.setdiff1d(np.arange(c.P), w.act)
    _bits(figs, tag + ".translation", a.poses[w.act, :3], w.poses[w.act, :3])
    n1, i1 = _mismatches(a.vel[w.act], w.vel[w.act])
    n2, _ = _mismatches(a.bias[w.act], w.bias[w.act])
    _fig(figs, tag + ".velocity_bias", n1 + n2, 0, i1)
    n = sum(_mismatches(x[inact], y[inact])[0] for x, y in ((a.poses, u.before.poses), (a.vel, u.before.vel), (a.bias, u.before.bias)))
    _fig(figs, tag + ".inactive_poses", n, 0)
    e, i = _worst(np.abs(np.asarray(a.poses[w.act, 3:7], dtype=LD) - w.quat[w.act]), np.full((len(w.act), 4), EPS))
    _fig(figs, tag + ".rotation", e, ROTATION_BOUND, int(w.act[i // 4]) if i >= 0 else -1)
    if c.LM == 3:
        _bits(figs, tag + ".landmarks", a.lms, w.lms)
    if c.LM == 1 and w.rho is not None:
        _bits(figs, tag + ".flags", a.rel, w.rel)
        if getattr(a, "rho", None) is not None:
            _bits(figs, tag + ".rho", a.rho, w.rho)
    elif c.LM == 3:
        _fig(figs, tag + ".flags", _mismatches(a.rel, u.before.rel)[0], 0)


def compare_world(figs, c, w):
    """x_w after end_solve against T_ws(reference pose after the update) x_s, x_s from the initial x_w and reference
    pose; rho0 (the device's inverse depth at begin_solve) against the same long-double x_s"""
    x_s, rho0, depth = world_to_sensor(c, w.x_w0, w.poses0, w.t_vs0)
    want, t_ref = sensor_to_world(c, x_s, w.rho1, w.poses1, w.t_vs1)
    tol = WORLD_BOUND * EPS * (np.sqrt((want * want).sum(-1)) + np.sqrt((t_ref * t_ref).sum(-1)))
    e, i = _worst(np.abs(np.asarray(w.x_w1[:, :3], dtype=LD) - want), np.repeat(tol, 3))
    _fig(figs, "world.xyz", e, 1.0, i // 3 if i >= 0 else -1)
    _bits(figs, "world.rho_bitwise", w.x_w1[:, 3], w.rho1)
    if getattr(w, "rho0", None) is not None:
        # the rigid transform leaves the inverse depth to the normalisation alone: rho = x_w[3] / |T_sw x_w|
        _, t0 = sensor_to_world(c, x_s, rho0, w.poses0, w.t_vs0)
        x0 = np.asarray(w.x_w0, dtype=LD)
        amp = (np.sqrt((x0[:, :3] ** 2).sum(-1)) + np.sqrt((t0 * t0).sum(-1)) * np.abs(x0[:, 3])) / (depth)
        e, i = _worst(np.abs(np.asarray(w.rho0, dtype=LD) - rho0), WORLD_BOUND * EPS * amp * np.abs(rho0))
        _fig(figs, "world.rho0", e, 1.0, i)


def compare(b, oracle_ratio=None, shards=1):
    """every figure of the bundle -> {name: namespace(value, bound, where)}; a figure holds when value <= bound.
    oracle_ratio: (landmark rows, pose rows) the oracle's own step reaches on this case; without it the two
    full-system figures are reported with an infinite bound."""
    c, figs = b.case, {}
    counts = chain_counts(c, shards)
    if getattr(b, "system", True) and getattr(b, "gn_l", None) is not None and getattr(b, "lin", None) is not None:
        (lm, lm_row), (pose, pose_row) = system_ratios(c, b.lin, b.gn_p, b.gn_l)
        bound = (np.inf, np.inf) if oracle_ratio is None else (SYSTEM_FACTOR * oracle_ratio[0], SYSTEM_FACTOR * oracle_ratio[1])
        _fig(figs, "system.landmark_rows", lm, bound[0], lm_row)
        if c.name.startswith("edges"):
            _fig(figs, "system.pose_rows", pose, bound[1], pose_row)
    for tag, ok in (("scal0", 0), ("scal1", 1)):
        got = getattr(b, tag, None)
        if got is None:
            continue
        ref = dogleg_reference(c, b.lin, b.rhs_p, b.rhs_l, b.gn_p, b.gn_l, ok)
        compare_scalars(figs, tag, c, got, ref, counts, getattr(b, "pp_jrhs", 0.0), getattr(b, "pp_tol", 0.0))
        if not ok:
            bad = [k for k in SCALARS if k.startswith("gn_") or k.startswith("rhs_gn_") if not got[k] == 0.0]
            _fig(figs, "scal0.gn_terms_zero", len(bad), 0, bad)
    for i, s in enumerate(getattr(b, "steps", ())):
        compare_step(figs, "step%d" % i, c, s, getattr(s, "rhs_p", b.rhs_p), getattr(s, "rhs_l", b.rhs_l), b.gn_p, b.gn_l, counts)
    for i, u in enumerate(getattr(b, "updates", ())):
        compare_update(figs, "update%d" % i, c, u)
    if getattr(b, "world", None) is not None:
        compare_world(figs, c, b.world)
    return figs


def failures(figs):
    return sorted(k for k, f in figs.items() if not f.value <= f.bound)


def worst(figs, prefix):
    """(name, figure) of the largest value / bound among the figures whose name starts with prefix"""
    best = None
    for k, f in figs.items():
        if k.startswith(prefix):
            q = f.value / f.bound if f.bound > 0 else (np.inf if f.value > 0 else 0.0)
            if best is None or q > best[0]:
                best = (q, k, f)
    return best[1:] if best else (None, None)


def report(name, figs):
    rows = []
    for prefix in ("system", "scal", "step", "update", "world"):
        k, f = worst(figs, prefix)
        if k:
            rows.append("%s %.3g (bound %.3g, at %s)" % (k, f.value, f.bound, f.where))
    print("STEP %s: %s" % (name, "; ".join(rows)), flush=True)


# ---- the float64 restatement ----------------------------------------------------------------------------------
MUTANTS = ("drop_block_last", "count_inactive_landmark", "jrhs_without_reference_pose", "jrhs_with_inactive_pose",
           "backsub_without_reference_row", "backsub_without_calibration", "step_by_landmark_id", "left_multiply",
           "sin_theta", "negative_kept", "revert_keeps_flag", "tail_in_norm", "zero_coefficient_reads_gn")


def _dense(c, J, idx):
    N = c.n + c.K + c.nl
    out = np.zeros((2 * c.O, N + 1))
    rows = np.arange(2 * c.O).reshape(c.O, 2)
    np.add.at(out, (rows[:, :, None], idx[:, None, :]), J)
    return out[:, :N]


def restate_solve(c, lin, gn_p, rhs_p=None, mutant=None):
    """rhs_p, rhs_l = J^T r and the back-substitution gn_l = V^-1 (rhs_l - W^T gn_p) in plain float64 from the
    per-residual inputs (dense J^T J).  The reduced solve itself is not part of the step path: gn_p is handed in.
    rhs_p is handed in where the pose-pose residuals add to it (vi15: they are not restated)."""
    idx, J = columns(c), local_jacobian(c, lin, np.float64)
    Jd = _dense(c, J, idx)
    r = np.asarray(lin.r, dtype=np.float64).reshape(-1)
    o = c.n + c.K
    H, g = Jd.T @ Jd, Jd.T @ r
    for i in masked_rows(c):
        H[i, :] = 0
        H[:, i] = 0
        H[i, i] = MASK_DIAGONAL
    _guard(H, c)
    W, V = H[:o, o:], H[o:, o:]
    Vi = np.zeros_like(V)
    for q in range(c.nl // c.LM):
        s = slice(q * c.LM, (q + 1) * c.LM)
        Vi[s, s] = np.linalg.inv(V[s, s])
    rhs_p = g[:o].copy() if rhs_p is None else np.asarray(rhs_p, dtype=np.float64)
    rhs_l = g[o:].copy()
    if mutant == "backsub_without_reference_row":
        J2 = J.copy()
        J2[:, :, 6:12] = 0
        W = (_dense(c, J2, idx).T @ Jd)[:o, o:]
    if mutant == "backsub_without_calibration":
        W = W.copy()
        W[c.n:] = 0
    gn_p = np.asarray(gn_p, dtype=np.float64)
    return rhs_p, rhs_l, gn_p, Vi @ (rhs_l - W.T @ gn_p)


def restate_scalars(c, lin, rhs_p, rhs_l, gn_p, gn_l, gn_ok, mutant=None):
    popt, lopt = opt_ids(c.pa), opt_ids(c.la)
    z = (lambda v: v) if gn_ok else np.zeros_like
    rp, rk, gp, gk, gl = rhs_p[:c.n], rhs_p[c.n:], z(gn_p[:c.n]), z(gn_p[c.n:]), z(gn_l)
    out = dict(rhs_p_sq=rp @ rp, gn_p_sq=gp @ gp, rhs_gn_p=rp @ gp, rhs_k_sq=rk @ rk, gn_k_sq=gk @ gk, rhs_gn_k=rk @ gk)
    # by landmark id, as the kernels walk them
    bl, gnl = np.zeros((c.L, c.LM)), np.zeros((c.L, c.LM))
    act = lopt >= 0
    bl[act], gnl[act] = rhs_l.reshape(-1, c.LM), gl.reshape(-1, c.LM)
    use = act.copy()
    if mutant == "drop_block_last":
        use[255::256] = False
    if mutant == "count_inactive_landmark":     # what a buffer that is not written for them may hold: a neighbour's value
        nxt = np.array([np.nonzero(act[l:])[0][0] + l if act[l:].any() else np.nonzero(act)[0][-1] for l in range(c.L)])
        bl[~act], gnl[~act] = bl[nxt[~act]], gnl[nxt[~act]]
        use[:] = True
    out.update(rhs_l_sq=(bl[use] ** 2).sum(), gn_l_sq=(gnl[use] ** 2).sum(), rhs_gn_l=(bl[use] * gnl[use]).sum())
    J, idx = local_jacobian(c, lin, np.float64), columns(c)
    grad = np.concatenate([rhs_p, rhs_l, [0.0]])
    if mutant == "jrhs_with_inactive_pose":     # an index of -1 taken for a pose: the last active one
        m = popt[c.pose]
        idx = idx.copy()
        idx[:, :6] = np.where(m[:, None] >= 0, idx[:, :6], (len(rp) // c.D - 1) * c.D + np.arange(6))
    T = J * grad[idx][:, None, :]
    if mutant == "jrhs_without_reference_pose":
        T[:, :, 6:12] = 0
    cal = np.zeros(T.shape[2], dtype=bool)
    cal[12:12 + c.K] = True
    v, u = T[:, :, ~cal].sum(2), T[:, :, cal].sum(2)
    out["j_rhs_sq"] = (v * v).sum() + (u * u).sum()
    return {k: float(v) for k, v in out.items()}


def restate_compose(c, a, b, rhs_p, rhs_l, gn_p, gn_l, mutant=None):
    """gn_p / gn_l: what the Gauss-Newton buffers hold (stale or NaN when b == 0: not to be read)"""
    lopt = opt_ids(c.la)
    read_gn = b != 0.0 or mutant == "zero_coefficient_reads_gn"
    step_p = a * rhs_p + (b * gn_p if read_gn else 0.0)
    val = a * rhs_l + (b * gn_l if read_gn else 0.0)
    step_l = val
    act = np.nonzero(lopt >= 0)[0]
    if mutant == "step_by_landmark_id":
        step_l = np.zeros_like(val).reshape(-1, c.LM)
        inside = act < len(step_l)
        step_l[act[inside]] = val.reshape(-1, c.LM)[inside]
        step_l = step_l.reshape(-1)
    used = val.reshape(-1, c.LM)
    if mutant == "drop_block_last":
        used = used[act % 256 != 255]
    end = len(step_p) if mutant == "tail_in_norm" else c.n
    return types.SimpleNamespace(a=a, b=b, step_p=step_p, step_l=step_l, norm_p=float(np.sqrt((step_p[:end] ** 2).sum())),
                                 norm_l=float(np.sqrt((used ** 2).sum())))


def restate_apply(c, before, step_p, step_l, mutant=None):
    popt, lopt = opt_ids(c.pa), opt_ids(c.la)
    act = np.nonzero(popt >= 0)[0]
    d = step_p[:c.n].reshape(-1, c.D)[popt[act]]
    a = types.SimpleNamespace(poses=before.poses.copy(), vel=before.vel.copy(), bias=before.bias.copy(), lms=None, rho=None,
                              rel=before.rel.copy())
    a.poses[act, :3] -= d[:, :3]
    qe = so3_exp_float64(-d[:, 3:6], sin_theta=mutant == "sin_theta")
    q = scene.quat_mul(qe, before.poses[act, 3:7]) if mutant == "left_multiply" else scene.quat_mul(before.poses[act, 3:7], qe)
    a.poses[act, 3:7] = q / np.sqrt((q * q).sum(-1, keepdims=True))
    if c.D >= 9:
        a.vel[act] -= d[:, 6:9]
    if c.D >= 15:
        a.bias[act] -= d[:, 9:15]
    la = np.nonzero(lopt >= 0)[0]
    dl = step_l.reshape(-1, c.LM)[lopt[la]]
    if c.LM == 3:
        a.lms = before.lms.copy()
        a.lms[la, :3] -= dl
    else:
        a.rho = before.rho.copy()
        moved = before.rho[la] - dl[:, 0]
        neg = moved < 0
        a.rho[la] = moved if mutant == "negative_kept" else np.where(neg, moved + dl[:, 0], moved)
        if mutant != "revert_keeps_flag":
            a.rel[la[neg]] = 0
    return a


def ladder_coefficients(c, gn_p):
    """b of compose_step(0, b) per rung: the largest rotation step of an active pose is the rung's angle"""
    rot = np.asarray(gn_p[:c.n]).reshape(-1, c.D)[:, 3:6]
    return [t / float(np.sqrt((rot * rot).sum(-1)).max()) for t in ROTATION_LADDER]


def negative_coefficient(c, rho, gn_l, fraction=0.25):
    """b that drives about `fraction` of the active landmarks' inverse depths below zero, none of them within 1e-6
    (relative) of it"""
    lopt = opt_ids(c.la)
    la = np.nonzero(lopt >= 0)[0]
    need = rho[la] / np.where(gn_l > 0, gn_l, np.inf)      # b above this turns the landmark negative
    need = np.sort(need[np.isfinite(need) & (need > 0)])
    k = max(1, int(len(need) * fraction))
    return float(0.5 * (need[k - 1] + need[k]))


def restate(c, lin, gn_p, rhs_p=None, rho0=None, mutant=None):
    """the whole step path in float64 from the per-residual inputs and the pose step of the reduced solve -> bundle.
    rho0: inverse depths at begin_solve (LmSize 1; default: the float64 world_to_sensor of the initial state)."""
    rhs_p, rhs_l, gn_p, gn_l = restate_solve(c, lin, gn_p, rhs_p, mutant)
    b = types.SimpleNamespace(case=c, lin=lin, rhs_p=rhs_p, rhs_l=rhs_l, gn_p=gn_p, gn_l=gn_l)
    b.scal0 = restate_scalars(c, lin, rhs_p, rhs_l, gn_p, gn_l, 0, mutant)
    b.scal1 = restate_scalars(c, lin, rhs_p, rhs_l, gn_p, gn_l, 1, mutant)
    state = initial_state(c)
    x_s = None
    if c.LM == 1:
        x_s, rho, _ = world_to_sensor(c, c.sc.landmarks, c.sc.poses, c.t_vs, np.float64)
        state.rho = rho if rho0 is None else rho0
    nan_p, nan_l = np.full_like(gn_p, np.nan), np.full_like(gn_l, np.nan)
    b.steps = [restate_compose(c, 0.3, 0.5, rhs_p, rhs_l, gn_p, gn_l, mutant),
               restate_compose(c, 0.7, 0.0, rhs_p, rhs_l, nan_p, nan_l, mutant)]
    coefs = ladder_coefficients(c, gn_p)
    if c.LM == 1:
        coefs.append(negative_coefficient(c, state.rho, gn_l))
    b.updates = []
    for k in coefs:
        s = restate_compose(c, 0.0, k, rhs_p, rhs_l, gn_p, gn_l, mutant)
        b.steps.append(s)
        b.updates.append(types.SimpleNamespace(step_p=s.step_p, step_l=s.step_l, before=state,
                                               after=restate_apply(c, state, s.step_p, s.step_l, mutant)))
    if c.LM == 1:       # one moderate step applied for real, then end_solve
        s = restate_compose(c, 0.0, 0.5, rhs_p, rhs_l, gn_p, gn_l, mutant)
        after = restate_apply(c, state, s.step_p, s.step_l, mutant)
        t_vs1 = exp_decoupled(c.t_vs, -s.step_p[c.n:]) if c.K else c.t_vs
        x_w1 = np.concatenate([sensor_to_world(c, x_s, after.rho, after.poses, t_vs1, np.float64)[0], after.rho[:, None]], 1)
        b.world = types.SimpleNamespace(x_w0=c.sc.landmarks, poses0=c.sc.poses, t_vs0=c.t_vs, poses1=after.poses, t_vs1=t_vs1,
                                        rho1=update_reference(c, state, s.step_p, s.step_l).rho, x_w1=x_w1, rho0=state.rho)
    return b


# ---- the oracle's side ----------------------------------------------------------------------------------------
def oracle_run(po, c, **options):
    """one Solve(1) of the oracle on case c at a fixed state (apply_results = 0, Gauss-Newton) -> namespace(lin, rhs_p,
    rhs_l, gn_p, gn_l, summary, ba): the per-residual inputs weighted by sqrt(w) and the vectors in the bundle's layout"""
    o = po.default_options()
    o.use_dogleg, o.error_change_threshold, o.param_change_threshold, o.apply_results = 0, 0, 0, 0
    o.enable_auto_regularization = 0
    for k, v in options.items():
        setattr(o, k, v)
    ba = po.OracleBundleAdjuster(c.LM, c.D, do_tvs=c.K == 6)
    ba.Init(o)
    sc = c.sc
    if c.imu:
        ba.SetGravity(sc.gravity)
    ba.AddCamera(sc.cam_params, c.t_vs)
    ba.add_poses(sc.poses, v_w=getattr(sc, "init_vel", None), b=getattr(sc, "init_bias", None), is_active=c.pa,
                 time=getattr(sc, "pose_time", None))
    ba.add_landmarks(sc.landmarks, sc.lm_ref_pose, is_active=c.la)
    ids = ba.add_projection_residuals(c.obs_z, c.obs_pose, c.obs_lm)
    if c.imu:
        for i in range(c.P - 1):
            ba.AddImuResidual(i, i + 1, sc.imu_meas[i])
    for args in c.regularize:
        ba.RegularizePose(*args)
    ba.Solve(1)
    assert ba.GetNumProjResiduals() == c.O
    sw = np.sqrt(ba.proj_weights())
    jm, jr, jl = ba.proj_jacobians()
    lin = types.SimpleNamespace(jm=jm * sw[:, None, None], jr=jr * sw[:, None, None], jl=jl * sw[:, None, None],
                                r=ba.proj_residuals() * sw[:, None], jk=None, w=ba.proj_weights())
    if c.K:
        lin.jk = ba.proj_tvs_jacobians() * sw[:, None, None]
    return types.SimpleNamespace(lin=lin, rhs_p=np.concatenate([ba.rhs_p(), ba.rhs_k()]), rhs_l=ba.rhs_l(),
                                 gn_p=np.concatenate([ba.delta_p(), ba.delta_k()]), gn_l=ba.delta_l(), summary=ba.summary(),
                                 ba=ba, ids=ids)
