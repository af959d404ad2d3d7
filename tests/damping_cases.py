"""Shared by the damping tests (test_damping.py, test_damping_gpu.py): the rules of ba_amd/csrc/damping.h restated in
numpy, the dense references of a damped step, and the call into the host restatement (ba_hostcheck_damping).
numpy only at import.

The damped step solves (H + lambda diag(d)) delta = g, d_j = min(max(H_jj, 1e-6), 1e32) for every free parameter and
d_j = 0 for a masked one (its 1e6 stays).  In the reduced form: V_lambda = V + lambda diag(d_l), S = U - W V_lambda^-1 W^T
+ lambda diag(clamp(diag U)), rhs = g_p - W V_lambda^-1 g_l, delta_l = V_lambda^-1 (g_l - W^T delta_p).  The predicted
decrease E(0) - E_model(delta) = 2 delta^T g - delta^T H delta = delta^T (lambda D delta + g)."""
import ctypes

import numpy as np

EPS = np.finfo(np.float64).eps
D_MIN, D_MAX = 1e-6, 1e32
LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12
MASKED = 1e6          # what a masked pose parameter carries on the diagonal of S


def hostcheck_damping(hc, op, values, lam=0.0, n=0, nout=1):
    """ba_hostcheck_damping(op, n, values, lambda) -> nout doubles"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    out = np.full(nout, np.nan)
    hc.ba_hostcheck_damping.restype = ctypes.c_int
    dp = ctypes.POINTER(ctypes.c_double)
    rc = hc.ba_hostcheck_damping(int(op), ctypes.c_uint32(n), v.ctypes.data_as(dp), ctypes.c_double(lam), out.ctypes.data_as(dp))
    assert rc == 0, rc
    return out


def clamp(h):
    return np.minimum(np.maximum(h, D_MIN), D_MAX)


def nielsen(lam, nu, rho):
    """(lambda, nu, accepted) after one gain ratio"""
    if rho > 0:
        return min(max(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), LAMBDA_MIN), LAMBDA_MAX), 2.0, True
    return min(max(lam * nu, LAMBDA_MIN), LAMBDA_MAX), 2.0 * nu, False


def damping_diagonal(H, masked=None):
    """d of the whole system: clamp(diag H) for free parameters, 0 for masked ones"""
    d = clamp(np.diag(H).copy())
    if masked is not None:
        d[masked] = 0.0
    return d


def dense_step(H, g, lam, masked=None):
    """(delta, d, predicted decrease) of the dense damped system; masked parameters carry 1e6 on the diagonal of H, no
    coupling and no right-hand side, as the engine leaves them"""
    d = damping_diagonal(H, masked)
    delta = np.linalg.solve(H + lam * np.diag(d), g)
    return delta, d, float(2.0 * delta @ g - delta @ H @ delta)


def reduced_step(H, g, n, lam, masked=None):
    """The same step through the reduced form of damping.h: the n pose parameters first, then the landmarks, whose
    block V is block diagonal.  -> (delta, S_lambda, rhs)"""
    U, W, V = H[:n, :n], H[:n, n:], H[n:, n:]
    gp, gl = g[:n], g[n:]
    Vl = V + lam * np.diag(clamp(np.diag(V)))
    Vi = np.linalg.inv(Vl) if V.size else V
    dp = clamp(np.diag(U).copy())
    if masked is not None:
        dp[masked[masked < n]] = 0.0
    S = U - W @ Vi @ W.T + lam * np.diag(dp)
    rhs = gp - W @ Vi @ gl
    delta_p = np.linalg.solve(S, rhs)
    delta_l = Vi @ (gl - W.T @ delta_p)
    return np.concatenate([delta_p, delta_l]), S, rhs


def random_ba_system(rng, n_pose=5, n_lm=12, lm_dim=3, D=6, obs_per_lm=3):
    """(H, g, n) of a random bundle-adjustment-shaped least-squares problem: H = J^T J + a small prior on the poses, V
    block diagonal, every landmark seen by obs_per_lm poses; g = J^T r"""
    n, nl = n_pose * D, n_lm * lm_dim
    rows = []
    for l in range(n_lm):
        for p in rng.choice(n_pose, size=obs_per_lm, replace=False):
            r = np.zeros((2, n + nl))
            r[:, p * D:(p + 1) * D] = rng.normal(size=(2, D))
            r[:, n + l * lm_dim:n + (l + 1) * lm_dim] = rng.normal(size=(2, lm_dim))
            rows.append(r)
    J = np.vstack(rows)
    res = rng.normal(size=J.shape[0])
    H = J.T @ J
    H[:n, :n] += 1e-3 * np.eye(n)
    return H, J.T @ res, n


# ---- the dense system of an engine's linearisation (test_damping_gpu.py) ---------------------------------------------
def engine_system(s, U_engine, rhs_p, rhs_l, pairs):
    """(H, g, n, masked) of the last UNDAMPED linearisation of the engine of a leverage_cases.Setup: the projection part
    J^T J from the engine's whitened Jacobians (leverage_cases.engine_jacobian: masked columns are zero, the listing rule
    applied); the pose-pose blocks as the difference between U_engine — the S of an engine on the same scene with every
    landmark inactive, where nothing is eliminated, so that no rounding of a Schur complement enters — and the pose
    part of J^T J, taken on the blocks of `pairs` only (pose ids (a, b) of every unary (a, a), binary and inertial
    residual) and exactly zero elsewhere; the fixed 1e6 of masked parameters; and g from the engine's unreduced
    right-hand sides (poses in the caller's order, landmarks by optimisation index)."""
    import leverage_cases as lc
    J, n = lc.engine_jacobian(s)
    Hp = J.T @ J
    Vg = guarded_v(Hp[n:, n:], s.lm_dim)
    H = Hp.copy()
    H[n:, n:] = Vg
    rows, D = lc.natural_rows(s.pa, s.D), s.D
    for a, b in pairs:
        for i, j in ((a, a), (b, b), (a, b), (b, a)):
            if rows[i] >= 0 and rows[j] >= 0:
                r, c = slice(rows[i], rows[i] + D), slice(rows[j], rows[j] + D)
                H[r, c] = Hp[r, c] + (U_engine[r, c] - Hp[r, c])
    masked = np.array([rows[p] + k for p in range(len(s.pa)) if s.pa[p] for k in range(s.D) if int(s.masks[p]) >> k & 1],
                      dtype=np.int64)
    H[masked, :] = 0.0
    H[:, masked] = 0.0
    H[masked, masked] = MASKED
    return H, np.concatenate([rhs_p, rhs_l]), n, masked


def pose_pose_pairs(pr):
    """pose ids (a, b) of every unary (a, a), binary and inertial residual of a Problem"""
    return [(int(p), int(p)) for p in pr.un] + [(int(a), int(b)) for a, b in zip(pr.b1, pr.b2)] + \
        [(int(a), int(b)) for a, b in zip(pr.i1, pr.i2)]


def guarded_v(V, lm_dim):
    """the 1e-6 guard of invert_v on every landmark block of V (an empty landmark has V = 0)"""
    V = V.copy()
    for k in range(0, V.shape[0], lm_dim):
        b = V[k:k + lm_dim, k:k + lm_dim]
        small = abs(b[0, 0]) < 1e-6 if lm_dim == 1 else np.linalg.norm(b) < 1e-6
        if small:
            b += 1e-6 * np.eye(lm_dim)
    return V


# ---- the scenes of test_damping_gpu.py: at the kernels' edges, not the workload's ---------------------------------
class Problem:
    """One problem: the scene, the accepted residuals (z, opose, olm), activity flags, masks and pose-pose residuals"""


EDGE_POSES = 12          # pose 0 is held fixed: 11 active poses x 6 = 66 rows of S, one past a 64-tile
BASE_LEN = 4
BACKGROUND = 40


def edge_lengths(lm_dim):
    """track lengths of tests/track_cases.py around the 64-observation range of a linearisation wave — 1 (LmSize 3: 2,
    one view leaves the 3 x 3 V singular), 2, 63, 64, 65 and 129 — an empty landmark, then the background"""
    return [1 if lm_dim == 1 else 2, 2, 63, 64, 65, 129, 0] + [BASE_LEN] * BACKGROUND


def _tracks(sc, lm_dim, lengths, seed):
    """the observation table of make_scene cut or extended to `lengths` accepted residuals per landmark, the way
    track_cases.build does it: shorter tracks drop observations, longer ones add observations (with replacement) from
    the poses that see the ground-truth point, measured with 1.5 px noise; shuffled with a fixed seed"""
    from ba_amd import scene
    L, P = len(lengths), sc.num_poses
    nsel = BASE_LEN + (1 if lm_dim == 1 else 0)
    first = nsel - BASE_LEN
    rng = np.random.Generator(np.random.PCG64([seed, 0xDA3F, lm_dim]))
    base_z, base_p = sc.obs_z.reshape(L, nsel, 2), sc.obs_pose.reshape(L, nsel)
    zs, ps, ls, refs = [], [], [], []
    for l in range(L):
        k = int(lengths[l])
        keep = first + min(k, BASE_LEN)
        zs.append(base_z[l, :keep])
        ps.append(base_p[l, :keep])
        ref = np.zeros(keep, dtype=bool)
        ref[:first] = True
        if k > BASE_LEN:
            uv, depth = scene.project(sc.gt_poses, np.broadcast_to(sc.gt_landmarks[l, :3], (P, 3)))
            vis = (depth > 0.5) & (uv[:, 0] > 0) & (uv[:, 0] < scene.IMG_W) & (uv[:, 1] > 0) & (uv[:, 1] < scene.IMG_H)
            vis[sc.lm_ref_pose[l]] = False
            cand = np.nonzero(vis)[0]
            assert len(cand) >= 2, "landmark %d is seen from %d poses only" % (l, len(cand))
            extra = rng.choice(cand, k - BASE_LEN, replace=True)
            zs.append(uv[extra] + rng.normal(0.0, 1.5, (len(extra), 2)))
            ps.append(extra.astype(base_p.dtype))
            ref = np.concatenate([ref, np.zeros(len(extra), dtype=bool)])
        refs.append(ref)
        ls.append(np.full(len(ref), l, dtype=np.uint32))
    z, pose, lm, ref = np.concatenate(zs), np.concatenate(ps).astype(np.uint32), np.concatenate(ls), np.concatenate(refs)
    perm = np.random.Generator(np.random.PCG64([seed, 0xDA3F, 99])).permutation(len(pose))
    z, pose, lm, ref = np.ascontiguousarray(z[perm]), pose[perm], lm[perm], ref[perm]
    acc = ~ref
    assert np.array_equal(np.bincount(lm[acc], minlength=L), lengths)
    return np.ascontiguousarray(z[acc]), np.ascontiguousarray(pose[acc]), np.ascontiguousarray(lm[acc])


def _relative(sc, a, b, rng):
    from ba_amd import scene
    Ra = scene.quat_to_rot(sc.gt_poses[a, 3:7])
    t = np.zeros(7)
    t[:3] = Ra.T @ (sc.gt_poses[b, :3] - sc.gt_poses[a, :3]) + 0.01 * rng.normal(size=3)
    t[3:7] = scene.quat_mul(sc.gt_poses[a, 3:7] * np.array([-1, -1, -1, 1]), sc.gt_poses[b, 3:7])
    return t


def edge_problem(lm_dim, seed=31):
    """11 active poses and one fixed (n = 66), the track lengths of edge_lengths, a pose with mask 0x7 and one with
    0x38, unary priors on three poses and binary edges with a duplicate, a reversed pair and one to the fixed pose,
    so that the pose diagonal U_jj has pose-pose parts"""
    from ba_amd import scene
    rng = np.random.default_rng(seed)
    pr = Problem()
    lengths = edge_lengths(lm_dim)
    P = EDGE_POSES
    sc = scene.make_scene(P, len(lengths), BASE_LEN, lm_dim=lm_dim, seed=seed, outlier_frac=0.0, anchors=(0,))
    pr.sc, pr.LM, pr.D, pr.P, pr.lengths = sc, lm_dim, 6, P, lengths
    pr.z, pr.opose, pr.olm = _tracks(sc, lm_dim, lengths, seed)
    pr.pa = np.ones(P, dtype=np.uint8)
    pr.pa[0] = 0
    pr.la = np.ones(len(lengths), dtype=np.uint8)
    pr.masks = np.zeros(P, dtype=np.uint16)
    pr.masks[3], pr.masks[5] = 0x7, 0x38
    pr.vel, pr.bias = np.zeros((P, 3)), np.zeros((P, 6))
    pr.un = np.array([2, 7, 9], dtype=np.uint32)
    pr.un_t = np.ascontiguousarray(sc.gt_poses[pr.un])
    pr.un_ci = np.ascontiguousarray(np.tile(np.diag([1e2] * 3 + [1e3] * 3).reshape(1, 36), (len(pr.un), 1)))
    edges = [(1, 2), (2, 3), (2, 3), (3, 2), (0, 1), (6, 7), (10, 11)]
    pr.b1 = np.array([e[0] for e in edges], dtype=np.uint32)
    pr.b2 = np.array([e[1] for e in edges], dtype=np.uint32)
    pr.b_t = np.ascontiguousarray(np.stack([_relative(sc, a, b, rng) for a, b in edges]))
    pr.b_ci = np.ascontiguousarray(np.tile(np.diag([50.0] * 6).reshape(1, 36), (len(edges), 1)))
    pr.b_cs = np.ascontiguousarray(np.tile(np.diag([np.sqrt(50.0)] * 6).reshape(1, 36), (len(edges), 1)))
    pr.i1 = pr.i2 = np.zeros(0, np.uint32)
    return pr


def inertial_problem(seed=5):
    """PoseSize 15, LmSize 1: 12 poses, the first fixed, 30 landmarks of 4 residuals, inertial residuals of 10 samples
    between neighbours and a unary prior: velocity and bias columns have no Schur part"""
    from ba_amd import scene
    rng = np.random.default_rng(seed)
    pr = Problem()
    P, L = 12, 30
    sc = scene.make_scene(P, L, 4, lm_dim=1, seed=seed, outlier_frac=0.0, anchors=(0,))
    scene.add_inertial(sc, period=60.0 * P / 100.0, seed=seed)
    pr.sc, pr.LM, pr.D, pr.P = sc, 1, 15, P
    sel = np.ones(len(sc.obs_pose), dtype=bool)
    sel[::5] = False
    pr.z, pr.opose, pr.olm = sc.obs_z[sel], sc.obs_pose[sel].astype(np.uint32), sc.obs_lm[sel].astype(np.uint32)
    pr.pa = np.ones(P, dtype=np.uint8)
    pr.pa[0] = 0
    pr.la = np.ones(L, dtype=np.uint8)
    pr.masks = np.zeros(P, dtype=np.uint16)
    pr.vel, pr.bias = sc.init_vel, 0.01 * rng.normal(size=(P, 6))
    pr.un = np.array([4], dtype=np.uint32)
    pr.un_t = np.ascontiguousarray(sc.gt_poses[pr.un])
    pr.un_ci = np.ascontiguousarray(np.tile(np.diag([1e2] * 3 + [1e3] * 3).reshape(1, 36), (1, 1)))
    pr.b1 = pr.b2 = np.zeros(0, np.uint32)
    pr.i1 = np.arange(0, P - 1, dtype=np.uint32)
    pr.i2 = pr.i1 + 1
    return pr


def singular_problem(seed=9):
    """All-active monocular scene (LmSize 1), only the root pose masked: the scale about the root is a free gauge, so
    the undamped S is singular to rounding"""
    from ba_amd import scene
    pr = Problem()
    P, L = 12, 60
    sc = scene.make_scene(P, L, 4, lm_dim=1, seed=seed, outlier_frac=0.0, anchors=(0,))
    pr.sc, pr.LM, pr.D, pr.P = sc, 1, 6, P
    sel = np.ones(len(sc.obs_pose), dtype=bool)
    sel[::5] = False
    pr.z, pr.opose, pr.olm = sc.obs_z[sel], sc.obs_pose[sel].astype(np.uint32), sc.obs_lm[sel].astype(np.uint32)
    pr.pa = np.ones(P, dtype=np.uint8)
    pr.la = np.ones(L, dtype=np.uint8)
    pr.masks = np.zeros(P, dtype=np.uint16)
    pr.masks[0] = 0x3f
    pr.vel, pr.bias = np.zeros((P, 3)), np.zeros((P, 6))
    pr.un = pr.b1 = pr.b2 = pr.i1 = pr.i2 = np.zeros(0, np.uint32)
    return pr
