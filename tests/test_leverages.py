"""Leverages of projection residuals on the CPU: leverage_host (ba_amd/csrc/lever.h, the plain C++ restatement of
k_lever.hip's formula and index logic, through ba_hostcheck_leverages) against a reference that uses no inverse —
the 2 x 2 diagonal blocks of Q Q^T for the thin QR of the dense whitened Jacobian.  Jacobians and weights from the
oracle; Sigma = inv(S) from numpy."""
import numpy as np
import pytest

from ba_amd import scene
from helpers import accepted_obs, fill, gn_options, hostcheck_lib
import leverage_cases as lc

SCENES = [(12, 60, 4), (30, 150, 5)]
_cache = {}


def _case(po, dims, lm_dim):
    """One linearisation of the oracle, the dense references and the host result: computed once, shared, read only."""
    key = (dims, lm_dim)
    if key in _cache:
        return _cache[key]
    sc = scene.make_scene(*dims, lm_dim=lm_dim, seed=21)
    pa = np.ones(sc.num_poses, dtype=np.uint8)
    pa[sc.anchor_poses] = 0
    la = np.ones(sc.num_landmarks, dtype=np.uint8)
    ba = po.OracleBundleAdjuster(lm_dim, 6)
    ba.Init(gn_options(po, apply_results=0))
    fill(ba, sc, active=pa)
    ba.Solve(1)
    jm, jr, jl = ba.proj_jacobians()
    w = ba.proj_weights()
    acc = np.array(accepted_obs(sc), dtype=np.int64)
    pp, pl = acc[:, 0], acc[:, 2]
    sw = np.sqrt(w)[:, None, None]
    J, n = lc.dense_jacobian(lm_dim, 6, 0, pa, la, sc.lm_ref_pose, pp, pl, sw * jm, sw * jr, sw * jl)
    S, sigma = lc.reduced_system(J, n)
    c = dict(sc=sc, pa=pa, la=la, pp=pp, pl=pl, jm=jm, jr=jr, jl=jl, w=w, J=J, n=n, S=S, sigma=sigma,
             want=lc.qr_blocks(J), lm_dim=lm_dim)
    c["got"] = _host(c, 0)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[key] = c
    return c


def _host(c, variant):
    return lc.host_leverages(hostcheck_lib(), c["lm_dim"], 6, 0, c["pa"], c["la"], c["sc"].lm_ref_pose, c["pp"], c["pl"],
                             c["jm"], c["jr"], c["jl"], None, c["w"], c["sigma"], variant)


@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("dims", SCENES)
def test_host_formula_equals_qr_blocks(oracle_lib, dims, lm_dim):
    c = _case(oracle_lib, dims, lm_dim)
    assert np.linalg.cond(c["S"]) < 1e7
    err = np.abs(c["got"] - c["want"]).max()
    print("max |H - QQ^T blocks| = %.3g over %d residuals" % (err, len(c["want"])))
    assert err <= 1e-10
    assert np.array_equal(c["got"], np.transpose(c["got"], (0, 2, 1)))


@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("dims", SCENES)
def test_traces_sum_to_the_unknown_count(oracle_lib, dims, lm_dim):
    c = _case(oracle_lib, dims, lm_dim)
    unknowns = c["J"].shape[1]
    assert unknowns == int(c["pa"].sum()) * 6 + lm_dim * c["sc"].num_landmarks
    tr = np.trace(c["got"], axis1=1, axis2=2).sum()
    print("sum tr H = %.12g, unknowns = %d" % (tr, unknowns))
    assert abs(tr - unknowns) <= 1e-8


@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("dims", SCENES)
def test_blocks_lie_between_zero_and_identity(oracle_lib, dims, lm_dim):
    c = _case(oracle_lib, dims, lm_dim)
    ev = np.linalg.eigvalsh(c["got"])
    print("eigenvalues in [%.3g, %.12g]" % (ev.min(), ev.max()))
    assert ev.min() >= -1e-10 and ev.max() <= 1 + 1e-10


@pytest.mark.parametrize("lm_dim,variant", [(1, 1), (3, 1), (1, 2), (3, 2), (1, 3)])
def test_wrong_variants_are_told_apart(oracle_lib, lm_dim, variant):
    """1: the sym2 cross term dropped; 2: Sigma_ll replaced by V^-1; 3: the reference-pose block of A dropped (LmSize 1).
    Each must miss the bound of test_host_formula_equals_qr_blocks."""
    for dims in SCENES:
        c = _case(oracle_lib, dims, lm_dim)
        err = np.abs(_host(c, variant) - c["want"]).max()
        print("variant %d: max error %.3g" % (variant, err))
        assert err > 1e-10
