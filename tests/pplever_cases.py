"""Shared by the tests of the pose-pose leverages (test_pose_pose_leverages.py, test_pose_pose_leverages_gpu.py):
the residual sets, their Jacobians from the oracle, the test's own effective informations Lambda, the dense whitened
Jacobian with its QR hat blocks, and the call into the host restatement (ba_hostcheck_pose_pose_leverages).
numpy only at import."""
import ctypes

import numpy as np

NONE = 0xFFFFFFFF
UNARY, BINARY, IMU = 0, 1, 2


class Terms:
    """unary | binary | inertial residuals of one problem, in the engine's slot order"""

    def __init__(self):
        self.un_pose = np.zeros(0, np.uint32)
        self.un_prior = np.zeros((0, 7))
        self.un_cov_inv = np.zeros((0, 6, 6))
        self.un_rot = np.zeros(0, np.uint8)
        self.bin_p1 = np.zeros(0, np.uint32)
        self.bin_p2 = np.zeros(0, np.uint32)
        self.bin_t12 = np.zeros((0, 7))
        self.bin_cov_inv = np.zeros((0, 6, 6))
        self.bin_sqrt = np.zeros((0, 6, 6))
        self.bin_w = np.zeros(0)
        self.bin_rot = np.zeros(0, np.uint8)
        self.imu_p1 = np.zeros(0, np.uint32)
        self.imu_p2 = np.zeros(0, np.uint32)

    @property
    def counts(self):
        return len(self.un_pose), len(self.bin_p1), len(self.imu_p1)

    @property
    def p1(self):
        return np.concatenate([self.un_pose, self.bin_p1, self.imu_p1]).astype(np.uint32)

    @property
    def p2(self):
        return np.concatenate([np.full(len(self.un_pose), NONE, np.uint32), self.bin_p2, self.imu_p2]).astype(np.uint32)

    def kind_slice(self, kind):
        nu, nb, ni = self.counts
        return [slice(0, nu), slice(nu, nu + nb), slice(nu + nb, nu + nb + ni)][kind]


def _relative(sc, a, b, noise):
    from ba_amd import scene
    Ra = scene.quat_to_rot(sc.gt_poses[a, 3:7])
    t = np.zeros(7)
    t[:3] = Ra.T @ (sc.gt_poses[b, :3] - sc.gt_poses[a, :3]) + noise
    t[3:7] = scene.quat_mul(sc.gt_poses[a, 3:7] * np.array([-1, -1, -1, 1]), sc.gt_poses[b, 3:7])
    return t


def helper_terms(sc, P, seed=3):
    """the residuals helpers._add_pose_pose gives an engine: unary priors on every 7th pose and odometry on every
    3rd neighbour pair (same values, same random draws)"""
    rng = np.random.default_rng(seed)
    t = Terms()
    t.un_pose = np.arange(0, P, 7, dtype=np.uint32)
    t.un_cov_inv = np.tile(np.diag([1e2] * 3 + [1e3] * 3), (len(t.un_pose), 1, 1))
    t.un_prior = np.ascontiguousarray(sc.gt_poses[t.un_pose])
    t.un_rot = np.ones(len(t.un_pose), np.uint8)
    t.bin_p1 = np.arange(0, P - 1, 3, dtype=np.uint32)
    t.bin_p2 = t.bin_p1 + 1
    nb = len(t.bin_p1)
    t.bin_t12 = np.stack([_relative(sc, a, b, 0.01 * rng.normal(size=3)) for a, b in zip(t.bin_p1, t.bin_p2)])
    t.bin_cov_inv = np.tile(np.diag([50.0] * 6), (nb, 1, 1))
    t.bin_sqrt = np.tile(np.diag([np.sqrt(50.0)] * 6), (nb, 1, 1))
    t.bin_w = np.ones(nb)
    t.bin_rot = np.ones(nb, np.uint8)
    return t


def _spd(rng, scale):
    """a 6 x 6 information matrix with off-diagonal terms, and its symmetric square root"""
    a = rng.normal(size=(6, 6))
    m = scale * (np.eye(6) + 0.1 * (a @ a.T) / 6.0)
    w, v = np.linalg.eigh(m)
    return m, (v * np.sqrt(w)) @ v.T


def pose_graph():
    """12 poses, PoseSize 6: unary priors on every 4th pose, odometry between neighbours, two loop closures (the
    second with use_rotation = 0 and weight 0.4; odometry 2 has weight 2.5); pose 5 inactive, pose 2 with its
    three translation parameters masked.  -> (scene, terms, pose_active, masks)"""
    from ba_amd import scene
    P = 12
    sc = scene.make_scene(P, 60, 4, lm_dim=1, seed=11)
    rng = np.random.default_rng(8)
    t = Terms()
    t.un_pose = np.arange(0, P, 4, dtype=np.uint32)
    t.un_cov_inv = np.stack([_spd(rng, 200.0)[0] for _ in t.un_pose])
    t.un_prior = np.ascontiguousarray(sc.gt_poses[t.un_pose])
    t.un_rot = np.ones(len(t.un_pose), np.uint8)
    pairs = [(i, i + 1) for i in range(P - 1)] + [(0, 7), (3, 11)]
    t.bin_p1 = np.array([a for a, _ in pairs], np.uint32)
    t.bin_p2 = np.array([b for _, b in pairs], np.uint32)
    t.bin_t12 = np.stack([_relative(sc, a, b, 0.01 * rng.normal(size=3)) for a, b in pairs])
    both = [_spd(rng, 50.0) for _ in pairs]
    t.bin_cov_inv = np.stack([m for m, _ in both])
    t.bin_sqrt = np.stack([s for _, s in both])
    t.bin_w = np.ones(len(pairs))
    t.bin_w[2], t.bin_w[-1] = 2.5, 0.4
    t.bin_rot = np.ones(len(pairs), np.uint8)
    t.bin_rot[-1] = 0
    pa = np.ones(P, np.uint8)
    pa[5] = 0
    masks = np.zeros(P, np.uint16)
    masks[2] = 0x7
    return sc, t, pa, masks


# Factors on the IMU noise options of the PoseSize 15 window.  tests/test_marginals_gpu.py widens gyro_sigma and
# accel_sigma by 10; on this window that leaves cond(S) = 7.5e6 (plain numpy), a bound of 7.5e-9 right under the
# 1e-8 gate: rotation and gyro bias carry 2e8 on the diagonal of S against 5e4 on the accelerometer bias.  With the
# gyro noise widened by 100 and the gyro bias walk by 10, cond(S) = 4.1e5.
IMU_NOISE_FACTORS = {"gyro_sigma": 100.0, "accel_sigma": 10.0, "gyro_bias_sigma": 10.0}


def widen_imu_noise(options):
    for k, f in IMU_NOISE_FACTORS.items():
        setattr(options, k, getattr(options, k) * f)
    return options


def imu_window(P=8):
    """PoseSize 15: P poses with an inertial residual per neighbour pair, a unary prior on every 3rd pose and
    odometry between neighbours; pose 0 inactive, so residual (0, 1) is the conditioning one whose dz1 block drops.
    -> (scene with pose times, velocities, samples, gravity; terms without Jacobians; pose_active, masks)"""
    from ba_amd import scene
    full = scene.make_scene(12, 60, 4, lm_dim=1, seed=2)   # (the generator needs more poses than the window has)
    scene.add_inertial(full, period=60.0 * 12 / 100.0)
    sc = scene.Scene()
    sc.num_poses = P
    sc.poses, sc.gt_poses = full.poses[:P].copy(), full.gt_poses[:P].copy()
    sc.init_vel, sc.init_bias, sc.pose_time = full.init_vel[:P].copy(), full.init_bias[:P].copy(), full.pose_time[:P].copy()
    sc.imu_meas, sc.gravity = full.imu_meas[:P - 1].copy(), full.gravity
    rng = np.random.default_rng(4)
    t = Terms()
    t.un_pose = np.arange(0, P, 3, dtype=np.uint32)
    t.un_cov_inv = np.tile(np.diag([1e2] * 3 + [1e3] * 3), (len(t.un_pose), 1, 1))
    t.un_prior = np.ascontiguousarray(sc.gt_poses[t.un_pose])
    t.un_rot = np.ones(len(t.un_pose), np.uint8)
    pairs = [(i, i + 1) for i in range(P - 1)]
    t.bin_p1 = np.array([a for a, _ in pairs], np.uint32)
    t.bin_p2 = t.bin_p1 + 1
    t.bin_t12 = np.stack([_relative(sc, a, b, 0.01 * rng.normal(size=3)) for a, b in pairs])
    t.bin_cov_inv = np.tile(np.eye(6), (len(pairs), 1, 1))
    t.bin_sqrt = np.tile(np.eye(6), (len(pairs), 1, 1))
    t.bin_w = np.ones(len(pairs))
    t.bin_rot = np.ones(len(pairs), np.uint8)
    t.imu_p1, t.imu_p2 = t.bin_p1.copy(), t.bin_p2.copy()
    pa = np.ones(P, np.uint8)
    pa[0] = 0
    return sc, t, pa, np.zeros(P, np.uint16)


def add_to_oracle(ba, sc, t):
    """the residuals through the reference-style API (oracle or adjuster): inertial, unary, binary"""
    for i in range(len(t.imu_p1)):
        ba.AddImuResidual(int(t.imu_p1[i]), int(t.imu_p2[i]), sc.imu_meas[int(t.imu_p1[i])])
    for i in range(len(t.un_pose)):
        ba.AddUnaryConstraint(int(t.un_pose[i]), t.un_prior[i], np.linalg.inv(t.un_cov_inv[i]), bool(t.un_rot[i]))
    for i in range(len(t.bin_p1)):
        ba.AddBinaryConstraint(int(t.bin_p1[i]), int(t.bin_p2[i]), t.bin_t12[i], np.linalg.inv(t.bin_cov_inv[i]),
                               float(t.bin_w[i]), bool(t.bin_rot[i]))


def add_to_engine(eng, t):
    """unary and binary residuals through the C-ABI (before finalize)"""
    c = np.ascontiguousarray
    dp, u32p, u8p = (ctypes.POINTER(x) for x in (ctypes.c_double, ctypes.c_uint32, ctypes.c_uint8))
    p = lambda a, ty: a.ctypes.data_as(ty)
    nu, nb, _ = t.counts
    a = [c(t.un_pose, np.uint32), c(t.un_prior), c(t.un_cov_inv.reshape(nu, 36)), c(t.un_rot, np.uint8)]
    eng._chk(eng.L.ba_hip_set_unary_residuals(eng.h, nu, p(a[0], u32p), p(a[1], dp), p(a[2], dp), p(a[3], u8p)))
    b = [c(t.bin_p1, np.uint32), c(t.bin_p2, np.uint32), c(t.bin_t12), c(t.bin_cov_inv.reshape(nb, 36)),
         c(t.bin_sqrt.reshape(nb, 36)), c(t.bin_w), c(t.bin_rot, np.uint8)]
    eng._chk(eng.L.ba_hip_set_binary_residuals(eng.h, nb, p(b[0], u32p), p(b[1], u32p), p(b[2], dp), p(b[3], dp),
                                               p(b[4], dp), p(b[5], dp), p(b[6], u8p)))


def oracle_jacobians(ba, t):
    """(dz (nres, 2, 15, 15) unmasked and unwhitened, imu cov_inv (ni, 15, 15)) of the oracle's last linearisation"""
    nu, nb, ni = t.counts
    dz = np.zeros((nu + nb + ni, 2, 15, 15))
    for i in range(nu):
        dz[i, 0, :6, :6] = ba.unary_jacobian(i)[0]
    for i in range(nb):
        a, b, _ = ba.binary_jacobians(i)
        dz[nu + i, 0, :6, :6], dz[nu + i, 1, :6, :6] = a, b
    ci = np.zeros((ni, 15, 15))
    for i in range(ni):
        dz[nu + nb + i, 0], dz[nu + nb + i, 1], ci[i], _ = ba.imu_jacobians(i)
    return dz, ci


def informations(t, un_scale=None, imu_cov_inv=None):
    """(info (nres, 15, 15) without the weight, weight (nres,)): Lambda = weight * info is the TEST's effective
    information — unary cov_inv * scale, binary weight * sqrt^T sqrt, inertial cov_inv"""
    nu, nb, ni = t.counts
    info = np.zeros((nu + nb + ni, 15, 15))
    w = np.ones(nu + nb + ni)
    info[:nu, :6, :6] = t.un_cov_inv
    if un_scale is not None:
        w[:nu] = un_scale
    info[nu:nu + nb, :6, :6] = np.einsum("nki,nkj->nij", t.bin_sqrt, t.bin_sqrt)
    w[nu:nu + nb] = t.bin_w
    if ni:
        info[nu + nb:] = imu_cov_inv
    return info, w


def res_dim(t, D):
    nu, nb, ni = t.counts
    return np.array([6] * (nu + nb) + [D] * ni)


def whitened_rows(t, D, dz, lam, pa, masks):
    """dense whitened Jacobian of the pose-pose residuals over the active poses in id order: rows G^T [dz1 | dz2]
    per residual (Lambda = G G^T, G the Cholesky factor of the test's Lambda), masked columns and inactive poses
    zero.  -> (J, row offsets (nres + 1), factors G)"""
    rows = natural_rows(pa, D)
    R = res_dim(t, D)
    off = np.concatenate([[0], np.cumsum(R)])
    J = np.zeros((off[-1], int(np.asarray(pa).sum()) * D))
    G = []
    for q, (a, b) in enumerate(zip(t.p1, t.p2)):
        g = np.linalg.cholesky(lam[q, :R[q], :R[q]])
        G.append(g)
        for side, p in enumerate((a, b)):
            if p == NONE or rows[p] < 0:
                continue
            blk = dz[q, side, :R[q], :D].copy()
            for c in range(D):
                if (int(masks[p]) >> c) & 1:
                    blk[:, c] = 0.0
            J[off[q]:off[q + 1], rows[p]:rows[p] + D] += g.T @ blk
    return J, off, G


def natural_rows(pa, D):
    opt = np.full(len(pa), -1, dtype=np.int64)
    opt[np.asarray(pa).astype(bool)] = np.arange(int(np.asarray(pa).sum()))
    return opt * D


def qr_blocks(Jfull, row0, off):
    """diagonal blocks of Q Q^T (thin QR of Jfull without its all-zero columns) for the residuals whose rows start at
    row0 + off[q]"""
    J = Jfull[:, np.abs(Jfull).max(0) > 0]
    Q = np.linalg.qr(J)[0]
    return [Q[row0 + off[q]:row0 + off[q + 1]] @ Q[row0 + off[q]:row0 + off[q + 1]].T for q in range(len(off) - 1)]


def whiten(C, G, R):
    """G^T C G per residual: the whitened hat blocks"""
    return [G[q].T @ C[q, :R[q], :R[q]] @ G[q] for q in range(len(G))]


def masked_diagonal(S, pa, masks, D):
    """S with the engine's 1e6 on the diagonal of the masked parameters"""
    S = S.copy()
    rows = natural_rows(pa, D)
    for p in range(len(pa)):
        for c in range(D):
            if rows[p] >= 0 and (int(masks[p]) >> c) & 1:
                S[rows[p] + c, rows[p] + c] += 1e6
    return S


def reference_cov(t, D, dz, pa, masks, sigma):
    """J Sigma_ee J^T per residual in numpy: (nres, 15, 15)"""
    rows = natural_rows(pa, D)
    out = np.zeros((len(t.p1), 15, 15))
    for q, (a, b) in enumerate(zip(t.p1, t.p2)):
        cols, blks = [], []
        for side, p in enumerate((a, b)):
            if p == NONE or rows[p] < 0:
                continue
            blk = dz[q, side, :, :D].copy()
            for c in range(D):
                if (int(masks[p]) >> c) & 1:
                    blk[:, c] = 0.0
            blks.append(blk)
            cols.append(np.arange(rows[p], rows[p] + D))
        if blks:
            Jq, ix = np.hstack(blks), np.concatenate(cols)
            out[q] = Jq @ sigma[np.ix_(ix, ix)] @ Jq.T
    return out


def host_leverages(hc, t, D, dz, info, weight, pa, masks, sigma, variant=0):
    """ba_hostcheck_pose_pose_leverages -> (cov (nres, 15, 15), Lambda (nres, 15, 15), leverage (nres,))"""
    c = lambda a, ty: np.ascontiguousarray(a, dtype=ty)
    p = lambda a, ty: a.ctypes.data_as(ctypes.POINTER(ty))
    dbl, u32, u16, u8 = ctypes.c_double, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint8
    pa, masks, p1, p2 = c(pa, np.uint8), c(masks, np.uint16), c(t.p1, np.uint32), c(t.p2, np.uint32)
    dz, info, weight, sigma = c(dz, np.float64), c(info, np.float64), c(weight, np.float64), c(sigma, np.float64)
    n = len(p1)
    cov, lam, lev = np.full((n, 15, 15), np.nan), np.full((n, 15, 15), np.nan), np.full(n, np.nan)
    hc.ba_hostcheck_pose_pose_leverages.restype = ctypes.c_int
    rc = hc.ba_hostcheck_pose_pose_leverages(D, len(pa), p(pa, u8), p(masks, u16), n, p(p1, u32), p(p2, u32), p(dz, dbl),
                                             p(info, dbl), p(weight, dbl), sigma.shape[0], p(sigma, dbl), int(variant),
                                             p(cov, dbl), p(lam, dbl), p(lev, dbl))
    assert rc == 0, rc
    return cov, lam, lev


def block_err(got, want):
    return max(np.abs(g - w).max() for g, w in zip(got, want))
