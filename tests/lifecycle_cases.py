"""Shared by the lifecycle tests (test_lifecycle.py, test_lifecycle_gpu.py): every lifecycle event of the engine
crossed with every reader of held device state (ba_amd/csrc/lifecycle.h, DESIGN.md "What the engine holds and what
drops it").

Two tables and one scene.  An EVENT is a short driver on hipapi.Engine plus the HeldEvent codes the engine fires while
it runs; a READER is a call on the engine plus the rule that says, from the Held bits, whether the engine serves it or
refuses it and with which message (the rules restate guard_kept_factor, guard_pcg_panel, the marginalize guard and
the guards of check_solve / get_S / get_pcg_stats of requests.h; test_lifecycle.py holds those guards to the rules).  The expected outcome of a cell is not written
down: walk() replays the codes fired so far through ba_hostcheck_lifecycle (the record of lifecycle.h itself, compiled
for the host) and applies the reader's rule to the bits that come back.  A cell is one of

  refuse     the reader raises HipError with the message of the branch (a regular expression of the wording)
  new        the system in A was rewritten since the first solve: the result is compared with a dense reference
  unchanged  nothing rewrote the system: the result equals the one taken before the event, bit for bit

The scene has two states A and B of identical structure (state B moves every free pose by a fixed perturbation), so a
stale read returns A's numbers where B's are due and stays inside its buffers.  numpy only at import."""
import ctypes

import numpy as np

from helpers import hostcheck_lib

# the enums HeldBit and HeldEvent of lifecycle.h, in their order
BITS = ("finalized", "snapshot", "err0", "err1", "lin", "dog_jrhs", "factored", "foreign", "pcg_solved", "pcg_last",
        "pcg_coarse_last", "sig", "pattern", "marg", "square_cleared")
EVENTS = ("problem_changed", "calibration_changed", "pose_cam_params_changed", "finalize_begins", "structure_rebuilt",
          "finalize_succeeded", "sharding_changed", "pattern_built", "solve_begins", "masks_changed", "linearize_begins",
          "linearize_writes_A", "linearize_succeeded", "gn_solve_begins", "solved_by_pcg", "solved_directly",
          "standalone_factorisation", "pcg_run_begins", "pcg_run_finished_plain", "pcg_run_finished_coarse",
          "dogleg_sums_ok", "dogleg_sums_failed", "step_applied_to_0", "step_applied_to_1", "rolled_back",
          "residuals_evaluated_at_0", "residuals_evaluated_at_1", "selinv_computed", "selinv_released",
          "marginalize_failed", "marginalized", "marginalization_released", "square_cleared", "square_dirty")


def replay(*events):
    """the set of held flags after each event, on a fresh record (ba_hostcheck_lifecycle)"""
    hc = hostcheck_lib()
    hc.ba_hostcheck_lifecycle.restype = ctypes.c_int
    ev = np.array([EVENTS.index(e) for e in events], dtype=np.int32)
    out = np.zeros(len(ev), dtype=np.uint32)
    rc = hc.ba_hostcheck_lifecycle(len(ev), ev.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    assert rc == 0, rc
    assert int(out.max()) < 1 << len(BITS)
    return [frozenset(b for i, b in enumerate(BITS) if v >> i & 1) for v in out]


def after(*events):
    return replay(*events)[-1] if events else frozenset()


# ---- the scene ---------------------------------------------------------------------------------------------------
P, L = 14, 60
FIXED = (0, 1)
# state B: every free pose moves by this much (metres; the rotation stays).  Chosen on the CPU
# (test_lifecycle.test_states_are_separated): every reader's dense reference at B lies more than 100 tolerances from
# the one at A.
SHIFT = 0.1


def scene_AB():
    """(scene, pose_active, (z, pose, lm) of the accepted residuals, poses of state A, poses of state B): the scene of
    test_lifecycle_gpu._scene — LmSize 1, 14 poses of which the first two are fixed (72 pose rows: two tiles), 60
    landmarks seen by 3 to 5 poses each — and a second state of the same structure."""
    from ba_amd import scene
    sc = scene.make_scene(P, L, 4, lm_dim=1, seed=11, anchors=FIXED)
    pa = np.ones(P, dtype=np.uint8)
    pa[list(FIXED)] = 0
    k = np.arange(len(sc.obs_pose)) % 5          # 0: the reference observation (rejected), 1 .. 4 accepted
    keep = (k >= 1) & (k <= 2 + sc.obs_lm % 3)
    obs = (sc.obs_z[keep], sc.obs_pose[keep], sc.obs_lm[keep])
    poses_a = np.ascontiguousarray(sc.poses, dtype=np.float64).copy()
    poses_b = poses_a.copy()
    d = np.random.default_rng(23).normal(size=(P, 3))
    d *= SHIFT / np.linalg.norm(d, axis=1)[:, None]
    poses_b[pa.astype(bool), :3] += d[pa.astype(bool)]
    return sc, pa, obs, poses_a, poses_b


# ---- messages: the wording of requests.h as regular expressions ----------------------------------------------------
NOT_FINALIZED = "ba_hip_finalize has not been called"
NO_FACTOR = "needs the factor of the last ba_hip_solve_gn \\(none yet, or the system was re-linearised since\\)"
NO_FACTOR_SHORT = "ba_hip_get_calibration_marginals needs the factor of the last ba_hip_solve_gn"
PCG_NO_FACTOR = "the last ba_hip_solve_gn ran the PCG solver \\(BA_HIP_SOLVER_PCG\\), which leaves no factor"
FOREIGN = "a stand-alone solve \\(ba_hip_tile_solve / ba_hip_dense_solve\\) has replaced the kept factor"
NO_LIN = "marginalize: needs the linearisation of the current state"
NO_CHECK = "ba_hip_check_solve needs keep_reduced_system and a finished ba_hip_solve_gn"
NO_PCG_STATS = "ba_hip_get_pcg_stats: the last ba_hip_solve_gn did not run the PCG solver"
DIRECT_HOLDS = "the last ba_hip_solve_gn ran the direct solver, A holds its factor and not S"
PCG_RELINEARISED = "the system was re-linearised since the PCG solve of the last ba_hip_solve_gn"
NO_PCG = "needs a PCG solve by the last ba_hip_solve_gn \\(BA_HIP_SOLVER_PCG; none yet"

# the kinds of refusal (test_lifecycle.test_every_refusal_kind_is_reached)
KINDS = {"not finalized": NOT_FINALIZED, "no factor": NO_FACTOR, "PCG left no factor": PCG_NO_FACTOR, "foreign factor": FOREIGN,
         "no linearisation": NO_LIN, "no PCG solve": NO_PCG, "direct solver holds the factor": DIRECT_HOLDS,
         "re-linearised since the PCG solve": PCG_RELINEARISED, "no finished solve": NO_CHECK, "no PCG statistics": NO_PCG_STATS}

SERVE = ("serve", None)


def refuse(kind, who=None, short=False):
    msg = KINDS[kind]
    if short and kind == "no factor":
        msg = NO_FACTOR_SHORT
    return ("refuse", kind, (who + ": " if who else "") + msg)


# ---- the rules: outcome from the Held bits, one per guard of requests.h -------------------------------------------
def rule_kept_factor(who, foreign_ok=lambda bits: False, short=False, honour=("finalized", "factored", "pcg_solved", "foreign")):
    """guard_kept_factor (with its finalized check).  honour: the bits the rule looks at — the negative
    check of test_lifecycle.py leaves one out and must see a cell change."""
    def rule(bits):
        has = lambda b: b in bits and b in honour
        if "finalized" in honour and "finalized" not in bits:
            return refuse("not finalized", None if short else who)
        if "factored" in honour and "factored" not in bits:
            if has("pcg_solved"):
                return refuse("PCG left no factor", who)
            return refuse("no factor", None if short else who, short)
        if has("foreign") and not foreign_ok(bits):
            return refuse("foreign factor", who)
        return SERVE
    return rule


def rule_marginals(who, **kw):
    """guard_marginals: a selected inverse computed before a stand-alone solve stays good"""
    return rule_kept_factor(who, foreign_ok=lambda bits: "sig" in bits, **kw)


def rule_pcg_panel(who):
    def rule(bits):
        if "finalized" not in bits:
            return refuse("not finalized", who)
        if "pcg_solved" not in bits:
            if "factored" in bits:
                return refuse("direct solver holds the factor", who)
            if "pcg_last" in bits:
                return refuse("re-linearised since the PCG solve", who)
            return refuse("no PCG solve", who)
        return SERVE
    return rule


def rule_marginalize(honour=("finalized", "lin")):
    def rule(bits):
        if "finalized" in honour and "finalized" not in bits:
            return refuse("not finalized")
        if "lin" in honour and "lin" not in bits:
            return refuse("no linearisation")
        return SERVE
    return rule


def rule_check_solve(bits):   # (every engine of these tests keeps the reduced system)
    if "finalized" not in bits:
        return refuse("not finalized")
    return SERVE if "pcg_solved" in bits or "factored" in bits else refuse("no finished solve")


def rule_get_S(bits):
    return SERVE if "finalized" in bits else refuse("not finalized")


def rule_pcg_stats(bits):
    return SERVE if "pcg_last" in bits else refuse("no PCG statistics")


# ---- the readers -----------------------------------------------------------------------------------------------------
RES_UNARY, RES_BINARY = 0, 1
POSE_IDS = [2, 9]
PAIR_A, PAIR_B = [2, 9], [9, 12]      # pose 12 holds rows 60 .. 65: its blocks straddle the two tiles
LM_IDS = [3, 40]
JOINT_IDS = [3, 11]
MARG_POSE = 5
MODES = 4
PCG_TOL = 1e-10
RHS = np.random.default_rng(29).standard_normal((6 * (P - len(FIXED)), 3))
RHS.setflags(write=False)


class Reader:
    """name; call(engine, ctx) -> a tuple of arrays (ctx: lev_ids, marg_lms); rule(bits) -> outcome; reads: the Held
    bits the rule looks at; fires(bits): the codes a served call fires; before: a driver run first (the cold variants
    of the marginal readers release the selected inverse) with the codes it fires."""

    def __init__(self, name, call, rule, reads, fires=lambda bits: (), before=None, before_codes=(), what="cov"):
        self.name, self.call, self.rule, self.reads, self.fires = name, call, rule, tuple(reads), fires
        self.before, self.before_codes, self.what = before, tuple(before_codes), what


def _selinv(bits):
    return () if "sig" in bits else ("selinv_computed",)


def _tup(x):
    return tuple(np.asarray(v) for v in x) if isinstance(x, tuple) else (np.asarray(x),)


def _marginal_readers():
    calls = [
        ("pose_marginals", "ba_hip_get_pose_marginals", lambda e, c: _tup(e.pose_marginals(POSE_IDS)), "pose"),
        ("pose_pair_marginals", "ba_hip_get_pose_pair_marginals", lambda e, c: _tup(e.pose_pair_marginals(PAIR_A, PAIR_B)), "pair"),
        ("landmark_marginals", "ba_hip_get_landmark_marginals", lambda e, c: _tup(e.landmark_marginals(LM_IDS)), "landmark"),
        ("projection_leverages", "ba_hip_get_projection_leverages", lambda e, c: _tup(e.projection_leverages(c["lev_ids"])), "lever"),
        ("pose_pose_leverages_unary", "ba_hip_get_pose_pose_leverages", lambda e, c: _tup(e.pose_pose_leverages(RES_UNARY)), "pp_unary"),
        ("pose_pose_leverages_binary", "ba_hip_get_pose_pose_leverages", lambda e, c: _tup(e.pose_pose_leverages(RES_BINARY)), "pp_binary"),
    ]
    reads = ("finalized", "factored", "pcg_solved", "foreign", "sig")
    warm = [Reader(n, f, rule_marginals(w), reads, _selinv, what=k) for n, w, f, k in calls]
    # without a prior compute_marginals: the selected inverse is released right before the call
    cold = [Reader(n + "_cold", f, rule_marginals(w), reads, _selinv, before=lambda e: e.release_marginals(),
                   before_codes=("selinv_released",), what=k) for n, w, f, k in calls[:3]]
    return warm, cold


def _marginalize(e, c):
    m = e.marginalize([MARG_POSE], c["marg_lms"])
    return (m["H"], m["b"], np.array([m["c"]]), m["x0"], m["pose_ids"].astype(np.float64))


def _readers():
    warm, cold = _marginal_readers()
    kf = ("finalized", "factored", "pcg_solved", "foreign")
    pcg = ("finalized", "factored", "pcg_solved", "pcg_last")
    rest = [
        Reader("joint_marginals", lambda e, c: _tup(e.joint_marginals(JOINT_IDS)), rule_kept_factor("ba_hip_get_joint_marginals"), kf,
               what="joint"),
        Reader("joint_state_marginals", lambda e, c: _tup(e.joint_state_marginals(POSE_IDS, LM_IDS)),
               rule_kept_factor("ba_hip_get_joint_state_marginals"), kf, what="joint_state"),
        Reader("factor_solve", lambda e, c: _tup(e.factor_solve(RHS)), rule_kept_factor("ba_hip_factor_solve"), kf, what="solve"),
        Reader("weakest_modes", lambda e, c: _tup(e.weakest_modes(MODES)), rule_kept_factor("ba_hip_get_weakest_modes"), kf,
               what="modes"),
        Reader("check_solve", lambda e, c: _tup(np.array(e.check_solve())), rule_check_solve, ("finalized", "factored", "pcg_solved"),
               what="check"),
        Reader("get_S", lambda e, c: _tup(e.get_S()), rule_get_S, ("finalized", "factored"), what="S"),
        Reader("marginalize", _marginalize, rule_marginalize(), ("finalized", "lin"), lambda bits: ("marginalized",), what="marg"),
        Reader("pcg_stats", lambda e, c: _tup(np.array([e.pcg_stats()[k] for k in ("iterations", "converged", "rel_residual_true")])),
               rule_pcg_stats, ("pcg_last",), what="pcg_stats"),
        Reader("pcg_panel_solve_system", lambda e, c: _tup(e.pcg_panel_solve_system(RHS, PCG_TOL)[0]),
               rule_pcg_panel("ba_hip_pcg_panel_solve_system"), pcg, what="pcg_solve"),
        Reader("joint_marginals_pcg", lambda e, c: _tup(e.joint_marginals_pcg(JOINT_IDS, rel_tolerance=PCG_TOL)),
               rule_pcg_panel("ba_hip_get_joint_marginals_pcg"), pcg, what="pcg_joint"),
    ]
    return warm + rest + cold   # (the cold variants last: they release the selected inverse the others may still hold)


READERS = _readers()
READER = {r.name: r for r in READERS}
CALIBRATION_READER = Reader("calibration_marginals", lambda e, c: _tup(e.get_calibration_marginals()),
                            rule_kept_factor("ba_hip_get_calibration_marginals", short=True),
                            ("finalized", "factored", "pcg_solved", "foreign"), what="calibration")


# ---- the events ------------------------------------------------------------------------------------------------------
UPLOAD = ("problem_changed",) * 6      # cameras, poses, landmarks, projection / unary / binary residuals
FINALIZE = ("finalize_begins", "structure_rebuilt", "finalize_succeeded")
LINEARIZE = ("linearize_begins", "linearize_writes_A", "pattern_built", "square_cleared", "linearize_succeeded")
DIRECT = ("gn_solve_begins", "solved_directly")
PCG = ("gn_solve_begins", "pcg_run_begins", "pcg_run_finished_plain", "solved_by_pcg")
# the first round of every engine: upload, finalize, begin_solve, masks, linearise, direct solve, compute_marginals
SETUP = UPLOAD + FINALIZE + ("solve_begins", "masks_changed") + LINEARIZE + DIRECT + ("selinv_computed",)
SETUP_PCG = UPLOAD + FINALIZE + ("solve_begins", "masks_changed") + LINEARIZE + PCG
SETUPS = {"direct": SETUP, "pcg": SETUP_PCG}
NEW_MASKS = {7: 0x7}   # pose 7 carries a unary prior and the odometry (6, 7): its translation gets masked


def _system(seed=5, n=65):
    """symmetric positive definite, every tile nonzero (the stand-alone solves)"""
    rng = np.random.default_rng(seed)
    m = rng.normal(size=(n, n))
    return m @ m.T + n * np.eye(n), rng.normal(size=n)


def _step(e):
    e.compose_step(0.0, 1.0)
    e.apply_step()


def _standalone(which):
    def run(e, c):
        A, b = _system()
        if which == "dense":
            assert e.dense_solve(np.tril(A), b)[1] == 0
        elif which == "tile":
            assert e.tile_solve(np.tril(A), b)[1] == 0
        else:
            assert e.pcg_solve(np.tril(A), b, 6, 1e-10)[1] == 0
    return run


def _masks(e, c):
    m = np.zeros(P, dtype=np.uint16)
    for p, v in NEW_MASKS.items():
        m[p] = v
    e.set_pose_masks(m)


def _solve_pcg(e, c):
    e.set_reduced_solver(1, rel_tolerance=PCG_TOL)
    e.linearize()
    assert e.solve_gn() == 0


def _pcg_then_direct(e, c):
    _solve_pcg(e, c)
    e.set_reduced_solver(0)
    e.linearize()
    assert e.solve_gn() == 0


def _pcg_then_linearize(e, c):
    _solve_pcg(e, c)
    e.linearize()


def _upload(e, c, bad=False):
    c["upload"](e, c["poses_a"], bad)


def _refinalize(e, c):
    _upload(e, c)
    e.finalize()


def _failed_finalize(e, c):
    _upload(e, c, bad=True)
    try:
        e.finalize()
    except Exception as x:   # (hipapi.HipError; this module does not import the binding)
        assert "projection residual references an unknown pose" in str(x), x
    else:
        raise AssertionError("the finalize of a residual that names pose %d was accepted" % P)


def _failed_then_good(e, c):
    _failed_finalize(e, c)
    _refinalize(e, c)


def _cam_params(e, c):
    e.set_pose_cam_params(np.tile(np.asarray(c["cam_params"], dtype=np.float64).ravel()[:4] * 1.01, (P, 1)))


class Event:
    """name; run(engine, ctx): the driver; codes: what the engine fires while it runs; restore(engine, ctx): puts the
    options back that the next round must not see; note: why a cell that may surprise is as it is; setup: the solver of
    the first round ("pcg": the readings before the event are those of a PCG solve)."""

    def __init__(self, name, run, codes, restore=None, note="", setup="direct"):
        self.name, self.run, self.codes, self.restore, self.note, self.setup = name, run, tuple(codes), restore, note, setup


EVENT_LIST = [
    Event("first_solve", lambda e, c: None, ()),
    Event("linearize", lambda e, c: e.linearize(), LINEARIZE),
    Event("apply_step", lambda e, c: _step(e), ("step_applied_to_1",)),
    Event("rollback", lambda e, c: (_step(e), e.rollback()), ("step_applied_to_1", "rolled_back")),
    Event("set_pose_masks", _masks, ("masks_changed",), restore=lambda e, c: e.set_pose_masks(np.zeros(P, dtype=np.uint16)),
          note="the new masks differ from those of the factored system: the pose-pose leverages must keep using the old ones"),
    Event("begin_solve", lambda e, c: e.begin_solve(), ("solve_begins",)),
    Event("dense_solve", _standalone("dense"), ("standalone_factorisation",)),
    Event("tile_solve", _standalone("tile"), ("standalone_factorisation",)),
    Event("pcg_solve", _standalone("pcg"), ("pcg_run_begins", "pcg_run_finished_plain"),
          note="a stand-alone PCG run has buffers of its own and touches neither the factor nor invdiag"),
    Event("solve_gn_pcg", _solve_pcg, LINEARIZE + PCG, restore=lambda e, c: e.set_reduced_solver(0)),
    Event("solve_gn_pcg_then_direct", _pcg_then_direct, LINEARIZE + PCG + LINEARIZE + DIRECT),
    Event("solve_gn_pcg_then_linearize", _pcg_then_linearize, LINEARIZE + PCG + LINEARIZE, restore=lambda e, c: e.set_reduced_solver(0)),
    Event("release_marginals", lambda e, c: e.release_marginals(), ("selinv_released",)),
    Event("release_marginalization", lambda e, c: e.release_marginalization(), ("marginalization_released",)),
    Event("set_pose_cam_params", _cam_params, ("pose_cam_params_changed",), restore=lambda e, c: e.set_pose_cam_params(None),
          note="the parameters take effect at the next linearisation; the rows marginalize absorbs are those of the last one"),
    Event("refinalize", _refinalize, UPLOAD + FINALIZE),
    Event("failed_finalize", _failed_finalize, UPLOAD + ("finalize_begins",)),
    Event("failed_then_good_finalize", _failed_then_good, UPLOAD + ("finalize_begins",) + UPLOAD + FINALIZE),
    # after a PCG solve_gn: S stays in A and the panel readers serve it
    Event("pcg:first_solve", lambda e, c: None, (), setup="pcg"),
    Event("pcg:apply_step", lambda e, c: _step(e), ("step_applied_to_1",), setup="pcg"),
    Event("pcg:set_pose_masks", _masks, ("masks_changed",), setup="pcg",
          restore=lambda e, c: e.set_pose_masks(np.zeros(P, dtype=np.uint16))),
    Event("pcg:dense_solve", _standalone("dense"), ("standalone_factorisation",), setup="pcg"),
    Event("pcg:pcg_solve", _standalone("pcg"), ("pcg_run_begins", "pcg_run_finished_plain"), setup="pcg",
          note="the stand-alone run takes the PCG work space; the panel solves upload their own tables"),
]
EVENT = {ev.name: ev for ev in EVENT_LIST}
REWRITES = ("linearize_writes_A", "finalize_begins")   # after these the system in A is not the one of the first solve


# ---- the derivation ----------------------------------------------------------------------------------------------------
class Cell:
    def __init__(self, event, reader, kind, refusal, message, bits):
        self.event, self.reader, self.kind, self.refusal, self.message, self.bits = event, reader, kind, refusal, message, bits

    def __repr__(self):
        return "%s x %s: %s%s" % (self.event, self.reader, self.kind, " (%s)" % self.refusal if self.refusal else "")


class Tracker:
    """the codes fired so far on one engine, and what a reader must do next"""

    def __init__(self, codes=()):
        self.codes = list(codes)

    def fire(self, *codes):
        self.codes += codes

    def bits(self):
        return after(*self.codes)

    def expect(self, reader, rule=None):
        """(outcome, bits) of the reader's next call; a served call fires the reader's own codes"""
        self.codes += reader.before_codes
        bits = self.bits()
        out = (rule or reader.rule)(bits)
        if out[0] == "serve":
            self.codes += reader.fires(bits)
        return out, bits


def walk(event, readers=None, rules=None, setup=None):
    """the cells of one event in the order the device test visits them: a generator of (reader, cell).  The codes of
    the first round, of the readings taken before the event (every reader once, in table order), of the event and of
    each reader visited so far are replayed on a fresh record; the reader's rule turns the bits into the outcome.
    rules: name -> rule, in place of the table's (the negative check)."""
    readers = READERS if readers is None else readers
    rules = rules or {}
    t = Tracker(SETUPS[event.setup] if setup is None else setup)
    for r in readers:   # the readings before the event
        t.expect(r)
    t.fire(*event.codes)
    rewritten = any(c in REWRITES for c in event.codes)
    for r in readers:
        out, bits = t.expect(r, rules.get(r.name))
        if out[0] == "serve":
            cell = Cell(event.name, r.name, "new" if rewritten else "unchanged", None, None, bits)
        else:
            cell = Cell(event.name, r.name, "refuse", out[1], out[2], bits)
        yield r, cell


def table(rules=None):
    """every cell of EVENT_LIST x READERS"""
    return [cell for ev in EVENT_LIST for _, cell in walk(ev, rules=rules)]


def matrix_markdown():
    """the event x reader matrix of DESIGN.md section 18 (python tests/lifecycle_cases.py prints it)"""
    short = {"not finalized": "R:fin", "no factor": "R:fac", "PCG left no factor": "R:pcg", "foreign factor": "R:for",
             "no linearisation": "R:lin", "no PCG solve": "R:nop", "direct solver holds the factor": "R:dir",
             "re-linearised since the PCG solve": "R:rel", "no finished solve": "R:chk", "no PCG statistics": "R:sta"}
    cells = table()
    lines = ["| reader \\ event | " + " | ".join("%d" % (i + 1) for i in range(len(EVENT_LIST))) + " |",
             "|---|" + "---|" * len(EVENT_LIST)]
    for r in READERS:
        row = []
        for ev in EVENT_LIST:
            c = next(x for x in cells if x.event == ev.name and x.reader == r.name)
            row.append({"new": "new", "unchanged": "same"}.get(c.kind) or short[c.refusal])
        lines.append("| `%s` | " % r.name + " | ".join(row) + " |")
    count = {k: sum(c.kind == k for c in cells) for k in ("refuse", "new", "unchanged")}
    legend = ["Events: " + ", ".join("%d `%s`" % (i + 1, ev.name) for i, ev in enumerate(EVENT_LIST)) + ".",
              "",
              "`new`: served and compared with a dense reference of the rewritten system; `same`: served bit for bit as "
              "before the event; " + ", ".join("`%s`: refused, %s" % (v, k) for k, v in short.items()) + ".",
              "",
              "%d cells: %d refuse, %d serve a new system, %d serve unchanged." % (len(cells), count["refuse"], count["new"],
                                                                                 count["unchanged"])]
    return "\n".join(legend + [""] + lines)


if __name__ == "__main__":
    print(matrix_markdown())
