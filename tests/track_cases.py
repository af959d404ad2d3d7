"""Graphs whose track lengths sit on the edges of the linearisation ranges, shared by tests/test_track_lengths.py
(host restatement, oracle soundness gate) and tests/test_track_lengths_gpu.py (device against the oracle).

ba_hip_finalize sorts the observations by landmark and packs whole landmarks into wavefront ranges of at most 64
observations; a landmark with more than 64 gets a range of its own, listed after the small ones and linearised by
the two-pass instantiation of k_linearize (ba_amd/csrc/structure.h, "linearisation waves").  The cases put track
lengths at 64, at sums of 64, just over 64, at multiples of 64 plus one, at zero, and leave shards without any short
track.  Measurements are real (true projections + 1.5 px noise), so residuals stay small, the Schur complement is
free of heavy cancellation and the tight tolerances of tests/test_gpu_parity.py apply.  Every case carries 600
background landmarks of length 6: without them many of the 180 poses see fewer than three points and S is singular
to working precision.  Numpy only."""
import numpy as np

from ba_amd import scene

NUM_POSES = 180
BACKGROUND = 600
BASE_LEN = 6
# chosen so that every pose is seen often enough: with this seed every active pose has at least 9 accepted
# observations in every case and for both LmSize values (asserted by the soundness gate of test_track_lengths.py)
SEED = 80


def expected_ranges(counts):
    """(n_small, n_big) of the packing rule: landmarks in id order, empty ones skipped; one with more than 64
    observations closes the open range and gets a range of its own; a range is closed before the landmark that
    would take it past 64."""
    n_small = n_big = cur = 0
    for k in counts:
        k = int(k)
        if k == 0:
            continue
        if k > 64:
            n_small += cur > 0
            n_big += 1
            cur = 0
            continue
        if cur + k > 64:
            n_small += 1
            cur = 0
        cur += k
    return n_small + (cur > 0), n_big


def prefixes(lm_dim):
    """name -> track lengths in front of the background.  LmSize 3 uses 2 where LmSize 1 uses 1: one view leaves
    the 3 x 3 V singular (guarded to inf on both sides)."""
    one = 1 if lm_dim == 1 else 2
    ones = [1] * 64 if lm_dim == 1 else [2] * 32
    return {
        "exact_64": [64, 64, 64],
        "packed_to_64": [32, 32, 16, 16, 16, 16, 63, one, 60, 4] + ones,
        "around_64": [63, 64, 65, one, 64, 66],
        "long_tracks": [65, 127, 128, 129, 200, 700],
        "long_tracks_odd": [65, 127, 128, 129, 200, 700, 66],   # the second wave of the last workgroup idles
        # zeros at the first id, between two landmarks of one range, directly before and after a long track
        "empty_landmarks": [0, 5, 0, 7, 0, 100, 0, 3],
    }


def cases(lm_dim):
    """name -> track length of every landmark (the named prefix, then the background)."""
    pre = prefixes(lm_dim)
    bg = [BASE_LEN] * BACKGROUND
    out = {k: v + bg for k, v in pre.items()}
    out["empty_landmarks"] = out["empty_landmarks"] + [0]     # ... and at the last id
    # the ranges start with long tracks, a long one closes an open small range half way, one is the last id
    out["only_long"] = [70, 300] + bg[:305] + [129] + bg[305:] + [65]
    out["mixed"] = (pre["exact_64"] + pre["packed_to_64"] + pre["around_64"] + pre["long_tracks_odd"]
                    + pre["empty_landmarks"] + bg[:305] + [129] + bg[305:] + [0, 65, 0])
    return out


# cases that are meant to reach the two-pass kernel
WITH_LONG = ("around_64", "long_tracks", "long_tracks_odd", "empty_landmarks", "only_long", "mixed")


def long_ids(lengths):
    return np.nonzero(np.asarray(lengths) > 64)[0]


def build(lm_dim, lengths, seed=SEED, outlier_frac=0.0, pixel_sigma=1.5, roll_amp=0.0):
    """-> (scene, z, pose, lm): landmark l has exactly lengths[l] ACCEPTED residuals.

    The scene is scene.make_scene(180, len(lengths), 6, ...) with its observation table replaced: shorter tracks
    drop observations; longer tracks add observations from poses that see the ground-truth point inside the image
    (depth > 0.5, the reference pose excluded), drawn with replacement — long tracks hold several observations
    from one pose — and measured as the true projection + N(0, pixel_sigma); `outlier_frac` of the added ones are
    gross mismatches, as in make_scene.  All observations are shuffled with a fixed seed: residual ids are not
    sorted by landmark.  scene.obs_* hold every observation (LmSize 1: with each landmark's reference observation,
    which sets z_ref and is rejected by AddProjectionResidual); (z, pose, lm) are the accepted ones in the same
    order, i.e. indexed by residual id.  roll_amp: the banked trajectory of the calibration tests."""
    lengths = np.asarray(lengths, dtype=np.int64)
    L = len(lengths)
    sc = scene.make_scene(NUM_POSES, L, BASE_LEN, lm_dim, seed, pixel_sigma=pixel_sigma, outlier_frac=outlier_frac,
                          roll_amp=roll_amp)
    nsel = BASE_LEN + (1 if lm_dim == 1 else 0)
    first = nsel - BASE_LEN                       # accepted observations of a landmark start here
    rng = np.random.Generator(np.random.PCG64([seed, 0x7ACC, lm_dim]))
    zs, ps, ls, refs = [], [], [], []
    base_z, base_p = sc.obs_z.reshape(L, nsel, 2), sc.obs_pose.reshape(L, nsel)
    for l in range(L):
        k = int(lengths[l])
        keep = first + min(k, BASE_LEN)
        zs.append(base_z[l, :keep])
        ps.append(base_p[l, :keep])
        ref = np.zeros(keep, dtype=bool)
        ref[:first] = True
        if k > BASE_LEN:
            x = sc.gt_landmarks[l, :3]
            uv, depth = scene.project(sc.gt_poses, np.broadcast_to(x, (NUM_POSES, 3)))
            vis = (depth > 0.5) & (uv[:, 0] > 0) & (uv[:, 0] < scene.IMG_W) & (uv[:, 1] > 0) & (uv[:, 1] < scene.IMG_H)
            vis[sc.lm_ref_pose[l]] = False
            cand = np.nonzero(vis)[0]
            assert len(cand) >= 3, "landmark %d is seen from %d poses only" % (l, len(cand))
            extra = rng.choice(cand, k - BASE_LEN, replace=True)
            ze = uv[extra] + rng.normal(0.0, pixel_sigma, (len(extra), 2))
            bad = rng.random(len(extra)) < outlier_frac
            zo = np.stack([rng.uniform(0, scene.IMG_W, len(extra)), rng.uniform(0, scene.IMG_H, len(extra))], -1)
            zs.append(np.where(bad[:, None], zo, ze))
            ps.append(extra.astype(base_p.dtype))
            ref = np.concatenate([ref, np.zeros(len(extra), dtype=bool)])
        refs.append(ref)
        ls.append(np.full(len(ref), l, dtype=np.uint32))
    z, pose, lm, ref = np.concatenate(zs), np.concatenate(ps).astype(np.uint32), np.concatenate(ls), np.concatenate(refs)
    perm = np.random.Generator(np.random.PCG64([seed, 0x7ACC, 99])).permutation(len(pose))
    z, pose, lm, ref = np.ascontiguousarray(z[perm]), pose[perm], lm[perm], ref[perm]
    sc.obs_z, sc.obs_pose, sc.obs_lm = z, pose, lm
    sc.obs_is_ref = ref
    sc.obs_per_landmark = None                    # no fixed count any more: helpers.accepted_obs does not apply
    sc.track_lengths = lengths
    acc = ~ref
    assert np.array_equal(np.bincount(lm[acc], minlength=L), lengths)
    return sc, np.ascontiguousarray(z[acc]), np.ascontiguousarray(pose[acc]), np.ascontiguousarray(lm[acc])


def symmetric(S):
    """the full matrix of an S kept in the upper triangle (use_triangular_matrices, the default)"""
    return np.triu(S) + np.triu(S, 1).T


def anchored(sc):
    """pose activity with the two gauge anchors held fixed (as test_reduced_system_and_step does)"""
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    return pa


def observations_per_active_pose(sc, pose, lm, pa):
    """accepted observations that touch each active pose: as measuring pose, or (LmSize 1) as reference pose"""
    cnt = np.bincount(pose, minlength=sc.num_poses)
    if sc.lm_dim == 1:
        cnt = cnt + np.bincount(sc.lm_ref_pose[lm], minlength=sc.num_poses)
    return cnt[pa.astype(bool)]
