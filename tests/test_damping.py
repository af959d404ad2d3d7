"""The Levenberg-Marquardt damping rules (ba_amd/csrc/damping.h) on the CPU, through ba_hostcheck_damping, and the new
engine fact GuardFacts::damped through ba_hostcheck_guard (bit 32 of its facts word).

numpy against numpy: the reduced form of the damped step (V + lambda diag(d_l), S_jj += lambda clamp(U_jj)) against the
dense (H + lambda D)^-1 g.  Both are backward-stable solves of the same system, so they agree to rounding: the bound
is REDUCED_BOUND cond_2(H + lambda D) eps on the relative error of delta, a small multiple of cond eps, not a measured
figure."""
import numpy as np
import pytest

import damping_cases as dc
import lifecycle_cases as lcs
from helpers import hostcheck_lib
from test_lifecycle import _ask_guard, KEPT_COPY, PLAN_FITS, HAS_OPTIONS, LANDMARKS

REDUCED_BOUND = 8.0     # multiples of cond(H + lambda D) eps
DAMPED = 32             # the new bit of the facts word
DAMPED_MSG = "the linearisation the device holds is damped (ba_hip_set_damping), linearise and solve once with damping 0"


@pytest.mark.parametrize("h, want", [(0.0, 1e-6), (1e-7, 1e-6), (1e-6, 1e-6), (1.0, 1.0), (1e32, 1e32), (1e33, 1e32)])
def test_clamp_rule(h, want):
    hc = hostcheck_lib()
    assert dc.hostcheck_damping(hc, 0, [h])[0] == want == dc.clamp(h)
    # the pose diagonal is the clamp of S_jj minus its Schur part
    assert dc.hostcheck_damping(hc, 4, [h - 0.25, -0.25])[0] == dc.clamp((h - 0.25) + 0.25)


@pytest.mark.parametrize("rho", [-1.0, 0.0, 0.25, 0.5, 0.75, 1.0])
def test_nielsen_update(rho):
    hc = hostcheck_lib()
    for lam, nu in ((1e-4, 2.0), (3.0, 8.0)):
        got = dc.hostcheck_damping(hc, 1, [lam, nu, rho], nout=3)
        wl, wn, wa = dc.nielsen(lam, nu, rho)
        assert got[2] == float(wa) == float(rho > 0)
        assert got[1] == wn
        assert abs(got[0] - wl) <= 4 * dc.EPS * wl
    if rho > 0:     # an accepted step never raises lambda by more than the factor 2 of rho -> 0, and resets nu
        assert got[0] <= 2.0 * lam and got[1] == 2.0
    else:
        assert got[0] == lam * nu and got[1] == 2 * nu
    if rho == 1.0:
        assert abs(got[0] - lam / 3.0) <= 4 * dc.EPS * lam
    if rho == 0.5:
        assert got[0] == lam


def test_nielsen_update_keeps_lambda_in_bounds():
    hc = hostcheck_lib()
    assert dc.hostcheck_damping(hc, 1, [dc.LAMBDA_MIN, 2.0, 1.0], nout=3)[0] == dc.LAMBDA_MIN     # would fall to a third
    assert dc.hostcheck_damping(hc, 1, [dc.LAMBDA_MAX, 2.0, -1.0], nout=3)[0] == dc.LAMBDA_MAX    # would double
    assert dc.hostcheck_damping(hc, 1, [dc.LAMBDA_MAX / 2, 64.0, 0.0], nout=3)[0] == dc.LAMBDA_MAX
    assert dc.hostcheck_damping(hc, 5, [0.0])[0] == dc.LAMBDA_MIN
    assert dc.hostcheck_damping(hc, 5, [1e13])[0] == dc.LAMBDA_MAX
    assert dc.hostcheck_damping(hc, 5, [0.5])[0] == 0.5
    # a NaN gain ratio (a step that left the domain) is a rejection
    got = dc.hostcheck_damping(hc, 1, [1.0, 2.0, np.nan], nout=3)
    assert got[2] == 0.0 and got[0] == 2.0 and got[1] == 4.0
    assert dc.hostcheck_damping(hc, 6, [10.0, 4.0, 3.0])[0] == 2.0


@pytest.mark.parametrize("lam", [1e-4, 1.0, 1e4])
def test_predicted_decrease_against_the_dense_model(lam):
    """delta^T (lambda D delta + g) of the host restatement against E(0) - E_model(delta) = 2 delta^T g - delta^T H delta
    of a random SPD system with a random g"""
    rng = np.random.default_rng(5)
    n = 40
    A = rng.normal(size=(2 * n, n))
    H = A.T @ A
    g = rng.normal(size=n)
    delta, d, want = dc.dense_step(H, g, lam)
    got = dc.hostcheck_damping(hostcheck_lib(), 2, np.concatenate([delta, g, d]), lam=lam, n=n, nout=2)
    cond = np.linalg.cond(H + lam * np.diag(d))
    # the two expressions are equal where (H + lambda D) delta = g holds; delta carries cond eps of relative error
    scale = abs(delta) @ (abs(H) @ abs(delta) + lam * d * abs(delta) + abs(g))
    print("lambda %g: pred %.6e, dense %.6e, |diff| / scale %.2e, cond %.2e" % (lam, got[1], want, abs(got[1] - want) / scale, cond))
    assert abs(got[1] - want) <= REDUCED_BOUND * cond * dc.EPS * scale
    assert abs(got[0] - delta @ (d * delta)) <= 4 * n * dc.EPS * got[0]
    assert want > 0


@pytest.mark.parametrize("lm_dim", [1, 3])
@pytest.mark.parametrize("lam", [1e-4, 1.0, 1e4])
def test_reduced_form_equals_the_dense_damped_step(lm_dim, lam):
    rng = np.random.default_rng(7 + lm_dim)
    H, g, n = dc.random_ba_system(rng, lm_dim=lm_dim)
    # one masked pose parameter, as the engine leaves it: no coupling, no right-hand side, 1e6 on the diagonal
    masked = np.array([4])
    H[masked, :] = 0.0
    H[:, masked] = 0.0
    H[masked, masked] = dc.MASKED
    g[masked] = 0.0
    dense, d, _ = dc.dense_step(H, g, lam, masked)
    red, S, rhs = dc.reduced_step(H, g, n, lam, masked)
    cond = np.linalg.cond(H + lam * np.diag(d))
    err = np.linalg.norm(red - dense) / np.linalg.norm(dense)
    print("LmSize %d lambda %g: |reduced - dense| / |dense| = %.2e, cond %.2e, bound %.2e" % (lm_dim, lam, err, cond, REDUCED_BOUND * cond * dc.EPS))
    assert err <= REDUCED_BOUND * cond * dc.EPS
    assert S[masked, masked] == dc.MASKED and red[masked] == 0.0
    # the damped V of the host restatement (guard, clamp, lambda d_l) is the V_lambda of the reduced form
    V = H[n:n + lm_dim, n:n + lm_dim]
    vs = V[np.triu_indices(lm_dim)]
    got = dc.hostcheck_damping(hostcheck_lib(), 3, vs, lam=lam, n=lm_dim, nout=len(vs) + lm_dim)
    want = (V + lam * np.diag(dc.clamp(np.diag(V))))[np.triu_indices(lm_dim)]
    assert np.abs(got[:len(vs)] - want).max() <= 2 * dc.EPS * np.abs(want).max()
    assert np.array_equal(got[len(vs):], dc.clamp(np.diag(V)))


def test_damped_v_applies_the_guard_first():
    """V = 0 (a landmark whose Jacobians vanish): the 1e-6 guard of invert_v, then d_l = 1e-6, then lambda d_l"""
    hc = hostcheck_lib()
    got = dc.hostcheck_damping(hc, 3, [0.0], lam=2.0, n=1, nout=2)
    assert got[1] == 1e-6 and got[0] == 1e-6 + 2.0 * 1e-6
    got = dc.hostcheck_damping(hc, 3, np.zeros(6), lam=2.0, n=3, nout=9)
    assert np.array_equal(got[6:], [1e-6] * 3)
    assert np.array_equal(got[:6], np.array([3e-6, 0, 0, 3e-6, 0, 3e-6]))


# ---- the new fact ------------------------------------------------------------------------------------------------
# (guard, who, noun, facts, flags, events, refused by the fact)
DIRECT, PCG = lcs.SETUP, lcs.SETUP_PCG
GUARDS = [
    ("kept_factor", "ba_hip_factor_solve", "solves with the factor", 0, 0, DIRECT, True),
    ("kept_factor", "ba_hip_get_calibration_marginals", None, 0, 0, DIRECT, False),
    ("marginals", "ba_hip_get_pose_marginals", None, 0, LANDMARKS, DIRECT, True),
    ("pcg_panel", "ba_hip_pcg_panel_solve_system", None, PLAN_FITS, HAS_OPTIONS, PCG, True),
    ("marginalize", "marginalize", None, 0, 0, DIRECT, True),
    ("check_solve", "", None, KEPT_COPY, 0, DIRECT, False),
    ("get_S", "", None, KEPT_COPY, 0, DIRECT, False),
    ("pcg_stats", "", None, 0, 0, PCG, False),
    ("pcg_coarse_stats", "", None, 0, 0,
     lcs.UPLOAD + lcs.FINALIZE + ("gn_solve_begins", "pcg_run_begins", "pcg_run_finished_coarse", "solved_by_pcg"), False),
]


@pytest.mark.parametrize("guard, who, noun, facts, flags, events, refused", GUARDS, ids=[g[0] + ("" if g[2] or g[0] != "kept_factor" else "_calibration") for g in GUARDS])
def test_the_damped_fact(guard, who, noun, facts, flags, events, refused):
    """each of the eight guards serves with the bit clear; with it set the readers of the kept factor, of the factor
    rows and of S for panel solves and marginalisation priors refuse with one sentence, the rest keep serving"""
    assert _ask_guard(events, guard, who, noun, facts, flags) == ""
    got = _ask_guard(events, guard, who, noun, facts | DAMPED, flags)
    if refused:
        assert got == who + ": " + DAMPED_MSG
    else:
        assert got == ""


def test_the_damped_fact_keeps_the_earlier_refusals_first():
    """not finalised and the sharded refusals are still named before the damping"""
    assert _ask_guard((), "kept_factor", "w", "weakest modes", DAMPED, 0) == "w: ba_hip_finalize has not been called"
    assert _ask_guard(DIRECT, "kept_factor", "w", "weakest modes", DAMPED | 1, 0) == "w: not available with the distributed solve"
    assert _ask_guard((), "marginalize", "", None, DAMPED, 0) == "ba_hip_finalize has not been called"
    # get_S serves the damped S whether or not the factor stands in A
    assert _ask_guard(lcs.UPLOAD + lcs.FINALIZE + lcs.LINEARIZE, "get_S", "", None, DAMPED, 0) == ""
