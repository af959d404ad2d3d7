"""The engine's lifecycle record (ba_amd/csrc/lifecycle.h) on the CPU: ba_hostcheck_lifecycle replays a list of
events on a fresh record and returns the flags after each one.  The sequences below are the event table of DESIGN.md
("What the engine holds and what drops it") stated as a test.  The second half derives the event x reader matrix of
lifecycle_cases.py from the same record: what test_lifecycle_gpu.py then asks of the engine."""
import ctypes

import numpy as np
import pytest

from helpers import hostcheck_lib

from lifecycle_cases import BITS, EVENTS   # the enums HeldBit and HeldEvent of lifecycle.h, in their order
import lifecycle_cases as lcs

FINALIZE = ("finalize_begins", "structure_rebuilt", "finalize_succeeded", "solve_begins", "masks_changed")
LINEARIZE = ("linearize_begins", "linearize_writes_A", "pattern_built", "square_cleared", "linearize_succeeded")
DIRECT = ("gn_solve_begins", "solved_directly")
PCG = ("gn_solve_begins", "pcg_run_begins", "pcg_run_finished_plain", "solved_by_pcg")


def replay(*events):
    """the set of held flags after each event"""
    hc = hostcheck_lib()
    hc.ba_hostcheck_lifecycle.restype = ctypes.c_int
    ev = np.array([EVENTS.index(e) for e in events], dtype=np.int32)
    out = np.zeros(len(ev), dtype=np.uint32)
    rc = hc.ba_hostcheck_lifecycle(len(ev), ev.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    assert rc == 0, rc
    assert int(out.max()) < 1 << len(BITS)
    return [{b for i, b in enumerate(BITS) if v >> i & 1} for v in out]


def after(*events):
    return replay(*events)[-1]


def test_codes_match_the_header():
    """every name above is a code of the header and the next code is none; a fresh record holds nothing but what the
    one event establishes"""
    hc = hostcheck_lib()
    hc.ba_hostcheck_lifecycle.restype = ctypes.c_int
    bad = np.array([0, len(EVENTS)], dtype=np.int32)
    out = np.zeros(2, dtype=np.uint32)
    assert hc.ba_hostcheck_lifecycle(2, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == -2
    establishes = {"finalize_succeeded": "finalized", "pattern_built": "pattern", "linearize_succeeded": "lin",
                   "solved_directly": "factored", "standalone_factorisation": "foreign", "dogleg_sums_ok": "dog_jrhs",
                   "pcg_run_finished_coarse": "pcg_coarse_last", "step_applied_to_0": "snapshot",
                   "step_applied_to_1": "snapshot", "residuals_evaluated_at_0": "err0", "residuals_evaluated_at_1": "err1",
                   "selinv_computed": "sig", "marginalized": "marg", "square_cleared": "square_cleared"}
    for e in EVENTS:
        want = {"pcg_solved", "pcg_last"} if e == "solved_by_pcg" else ({establishes[e]} if e in establishes else set())
        assert after(e) == want, e


def test_refinalize_after_a_direct_solve():
    seq = FINALIZE + LINEARIZE + DIRECT + ("selinv_computed",)
    held = after(*seq)
    assert {"finalized", "factored", "lin", "sig", "pattern"} <= held and "foreign" not in held
    changed = after(*seq, "problem_changed")
    assert changed == held - {"finalized"}
    again = after(*seq, "problem_changed", "finalize_begins")
    assert again == held - {"finalized", "factored", "sig", "lin"}
    # a finalize that fails midway leaves the engine unfinalised; one that succeeds rebuilds pattern and square
    assert "finalized" not in after(*seq, "finalize_begins", "structure_rebuilt")
    done = after(*seq, "finalize_begins", "structure_rebuilt", "finalize_succeeded")
    assert done == {"finalized"}


def test_refinalize_keeps_the_facts_about_the_last_solve():
    """factor_foreign, pcg_last / pcg_coarse_last and the marginalisation result survive "finalize begins"; the PCG
    solution does not"""
    seq = FINALIZE + LINEARIZE + ("gn_solve_begins", "pcg_run_begins", "pcg_run_finished_coarse", "solved_by_pcg",
                                  "marginalized", "standalone_factorisation")
    held = after(*seq)
    assert {"pcg_solved", "pcg_last", "pcg_coarse_last", "marg", "foreign"} <= held
    again = after(*seq, "finalize_begins")
    assert {"pcg_last", "pcg_coarse_last", "marg", "foreign"} <= again and "pcg_solved" not in again


def test_standalone_factorisation():
    seq = FINALIZE + LINEARIZE + DIRECT + ("selinv_computed", "standalone_factorisation")
    held = after(*seq)
    assert {"sig", "foreign", "factored"} <= held
    again = after(*seq, *DIRECT)
    assert "sig" not in again and "foreign" not in again and "factored" in again


def test_pcg_solve():
    seq = FINALIZE + LINEARIZE + PCG
    held = after(*seq)
    assert {"pcg_solved", "pcg_last"} <= held and "factored" not in held and "pcg_coarse_last" not in held
    assert "pcg_coarse_last" in after(*FINALIZE, *LINEARIZE, "gn_solve_begins", "pcg_run_begins",
                                      "pcg_run_finished_coarse", "solved_by_pcg")
    relin = after(*seq, "linearize_begins", "linearize_writes_A")
    assert relin == held - {"pcg_solved", "lin"}
    # the next direct solve forgets that PCG ran
    assert not {"pcg_solved", "pcg_last"} & after(*seq, *DIRECT)


def test_failed_linearize_keeps_the_factor():
    seq = FINALIZE + LINEARIZE + DIRECT + ("dogleg_sums_ok",)
    held = after(*seq)
    assert {"factored", "dog_jrhs", "lin"} <= held
    assert after(*seq, "linearize_begins") == held - {"dog_jrhs"}
    assert after(*seq, "linearize_begins", "linearize_writes_A") == held - {"dog_jrhs", "factored", "lin"}


def test_step_and_rollback():
    seq = FINALIZE + LINEARIZE + DIRECT + ("residuals_evaluated_at_0", "step_applied_to_1", "residuals_evaluated_at_1")
    steps = replay(*seq)
    assert "lin" in steps[-3] and "lin" not in steps[-2] and "snapshot" in steps[-2]
    held = steps[-1]
    assert {"err0", "err1", "snapshot", "factored"} <= held
    relin = after(*seq, *LINEARIZE)
    assert {"err0", "err1", "lin", "snapshot"} <= relin
    second = after(*seq, *LINEARIZE, "step_applied_to_0")
    assert second == relin - {"err0", "lin"}
    back = after(*seq, *LINEARIZE, "rolled_back")
    assert back == relin - {"snapshot", "lin"}


def test_masks_keep_the_factor():
    seq = FINALIZE + LINEARIZE + DIRECT + ("dogleg_sums_ok",)
    held = after(*seq)
    assert after(*seq, "masks_changed") == held - {"dog_jrhs", "lin"}


def test_begin_solve_and_sharding():
    seq = FINALIZE + LINEARIZE + DIRECT + ("dogleg_sums_ok", "residuals_evaluated_at_0", "step_applied_to_1",
                                           "residuals_evaluated_at_1", "selinv_computed")
    held = after(*seq)
    assert {"err0", "err1", "dog_jrhs", "pattern", "factored", "sig"} <= held
    assert after(*seq, "solve_begins") == held - {"err0", "err1", "dog_jrhs"}
    assert after(*seq[:-4], "solve_begins") == after(*seq[:-4]) - {"dog_jrhs", "lin"}   # (before the step: lin held)
    assert after(*seq, "sharding_changed") == held - {"pattern", "dog_jrhs"}


@pytest.mark.parametrize("event,drops", [
    ("calibration_changed", {"finalized", "dog_jrhs"}),
    ("pose_cam_params_changed", {"err0", "err1"}),
    ("dogleg_sums_failed", {"dog_jrhs"}),
    ("selinv_released", {"sig"}),
    ("marginalize_failed", {"marg"}),
    ("marginalization_released", {"marg"}),
    ("square_dirty", {"square_cleared"}),
    ("structure_rebuilt", {"pattern", "snapshot", "square_cleared"}),
])
def test_single_drops(event, drops):
    seq = FINALIZE + LINEARIZE + DIRECT + ("dogleg_sums_ok", "residuals_evaluated_at_0", "step_applied_to_1",
                                           "residuals_evaluated_at_1", "selinv_computed", "marginalized")
    held = after(*seq)
    assert drops <= held
    assert after(*seq, event) == held - drops


# ---- the event x reader matrix (lifecycle_cases.py; the device side is test_lifecycle_gpu.py) ------------------
def test_the_tables_name_codes_of_the_header():
    for ev in lcs.EVENT_LIST:
        assert set(ev.codes) <= set(EVENTS), ev.name
    for r in lcs.READERS + [lcs.CALIBRATION_READER]:
        assert set(r.reads) <= set(BITS) and set(r.before_codes) <= set(EVENTS), r.name
    assert len({ev.name for ev in lcs.EVENT_LIST}) == len(lcs.EVENT_LIST)
    assert len({r.name for r in lcs.READERS}) == len(lcs.READERS)


def test_every_cell_is_decided_by_the_bits_its_reader_reads():
    """For every event sequence of the table the replayed bits give the reader's rule all it needs: the outcome does
    not move when any bit outside reader.reads is flipped, and it is a refusal with a message or a plain serve."""
    cells = lcs.table()
    assert len(cells) == len(lcs.EVENT_LIST) * len(lcs.READERS)
    for c in cells:
        r = lcs.READER[c.reader]
        base = r.rule(c.bits)
        assert base[0] in ("serve", "refuse") and (base[0] == "serve" or (base[1] in lcs.KINDS and base[2]))
        for b in set(BITS) - set(r.reads):
            assert r.rule(c.bits ^ {b}) == base, (c, b)


def test_every_reader_is_reached_in_every_way_its_rule_allows():
    """refuse, serve a new system, serve unchanged: each at least once per reader; a kind that no event / reader pair
    reaches is reported."""
    cells = lcs.table()
    missing = [(r.name, k) for r in lcs.READERS for k in ("refuse", "new", "unchanged")
               if not any(c.reader == r.name and c.kind == k for c in cells)]
    assert not missing, missing


# the refusal kinds each reader's guard can produce (the sharded / distributed branches are out of scope)
CAN_REFUSE = {
    "kept factor": ("not finalized", "no factor", "PCG left no factor", "foreign factor"),
    "panel": ("not finalized", "no PCG solve", "direct solver holds the factor", "re-linearised since the PCG solve"),
    "marginalize": ("not finalized", "no linearisation"),
    "check_solve": ("not finalized", "no finished solve"),
    "get_S": ("not finalized",),
    "pcg_stats": ("no PCG statistics",),
}


def _guard(name):
    if name in ("marginalize", "check_solve", "get_S", "pcg_stats"):
        return name
    return "panel" if name in ("pcg_panel_solve_system", "joint_marginals_pcg") else "kept factor"


def test_every_refusal_kind_is_reached():
    """not finalized, no factor, PCG left no factor, foreign factor, no linearisation, no PCG solve, direct solver
    holds the factor (and the third message of pcg_panel_ready): by at least one cell per reader that can produce
    it.  The marginal readers reach "foreign factor" through their cold variant or after release_marginals."""
    cells = lcs.table()
    got = {}
    for c in cells:
        if c.kind == "refuse":
            got.setdefault(c.reader[:-5] if c.reader.endswith("_cold") else c.reader, set()).add(c.refusal)
    # the leverages have no cold variant of their own: after release_marginals + a stand-alone solve they refuse too
    t = lcs.Tracker(lcs.SETUP + ("standalone_factorisation", "selinv_released"))
    for r in lcs.READERS:
        if r.reads == lcs.READER["pose_marginals"].reads and not r.before:
            out, _ = t.expect(r)
            assert out[:2] == ("refuse", "foreign factor"), r.name
            got.setdefault(r.name, set()).add(out[1])
    for r in lcs.READERS:
        if r.before:
            continue
        want = set(CAN_REFUSE[_guard(r.name)])
        assert want <= got.get(r.name, set()), (r.name, want - got.get(r.name, set()))
    for kind in ("not finalized", "no factor", "PCG left no factor", "foreign factor", "no linearisation", "no PCG solve",
                 "direct solver holds the factor"):
        assert any(c.refusal == kind for c in cells), kind


@pytest.mark.parametrize("drop,readers", [
    ("foreign", ("joint_marginals", "factor_solve", "weakest_modes", "joint_state_marginals", "pose_marginals_cold")),
    ("factored", ("pose_marginals", "factor_solve")),
    ("pcg_solved", ("landmark_marginals", "joint_marginals")),
    ("finalized", ("projection_leverages", "weakest_modes")),
    ("lin", ("marginalize",)),
])
def test_a_rule_that_ignores_a_flag_is_noticed(drop, readers):
    """The negative check: a reader rule that does not look at factor_foreign, lin_valid (or factored, pcg_solved,
    finalized) derives a matrix that differs from the table's in at least one cell of that reader."""
    want = {(c.event, c.reader): (c.kind, c.refusal) for c in lcs.table()}
    for name in readers:
        r = lcs.READER[name]
        if name == "marginalize":
            blind = lcs.rule_marginalize(honour=tuple(b for b in ("finalized", "lin") if b != drop))
        else:
            honour = tuple(b for b in ("finalized", "factored", "pcg_solved", "foreign") if b != drop)
            who = "x"
            blind = (lcs.rule_marginals if "sig" in r.reads else lcs.rule_kept_factor)(who, honour=honour)
        got = {(c.event, c.reader): (c.kind, c.refusal) for c in lcs.table(rules={name: blind})}
        differ = [k for k in want if k[1] == name and want[k] != got[k]]
        assert differ, "no cell of %s notices a rule without %s" % (name, drop)


def test_documented_matrix_is_the_derived_one():
    """DESIGN.md section 18 holds the matrix as lifecycle_cases.matrix_markdown() prints it"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "DESIGN.md"), encoding="utf-8") as f:
        doc = f.read()
    assert lcs.matrix_markdown() in doc


# ---- the guards of requests.h themselves (ba_hostcheck_guard) against the readers' rules -------------------------
KEPT_COPY, PLAN_FITS = 8, 16                 # facts: every engine of these tests keeps the reduced system
FOREIGN_OK, LANDMARKS, HAS_OPTIONS = 1, 2, 4   # flags


def _guard_of(reader):
    """(guard, who, noun, facts, flags) of ba_hostcheck_guard for a reader of the table"""
    name = reader.name[:-5] if reader.name.endswith("_cold") else reader.name
    kept = {"joint_marginals": ("ba_hip_get_joint_marginals", "joint marginals", 0),
            "joint_state_marginals": ("ba_hip_get_joint_state_marginals", "joint marginals", LANDMARKS),
            "factor_solve": ("ba_hip_factor_solve", "solves with the factor", 0),
            "weakest_modes": ("ba_hip_get_weakest_modes", "weakest modes", 0)}
    marginals = {"pose_marginals": ("ba_hip_get_pose_marginals", 0), "pose_pair_marginals": ("ba_hip_get_pose_pair_marginals", 0),
                 "landmark_marginals": ("ba_hip_get_landmark_marginals", LANDMARKS),
                 "projection_leverages": ("ba_hip_get_projection_leverages", LANDMARKS),
                 "pose_pose_leverages_unary": ("ba_hip_get_pose_pose_leverages", 0),
                 "pose_pose_leverages_binary": ("ba_hip_get_pose_pose_leverages", 0)}
    panel = {"pcg_panel_solve_system": "ba_hip_pcg_panel_solve_system", "joint_marginals_pcg": "ba_hip_get_joint_marginals_pcg"}
    if name in kept:
        return ("kept_factor", kept[name][0], kept[name][1], 0, kept[name][2])
    if name in marginals:
        return ("marginals", marginals[name][0], None, 0, marginals[name][1])
    if name in panel:
        return ("pcg_panel", panel[name], None, PLAN_FITS, HAS_OPTIONS)
    if name == "calibration_marginals":
        return ("kept_factor", "ba_hip_get_calibration_marginals", None, 0, 0)
    assert name in ("check_solve", "get_S", "marginalize", "pcg_stats"), name
    return (name, "", None, KEPT_COPY, 0)


def _ask_guard(codes, guard, who, noun, facts, flags):
    """the message of the C++ guard after the events `codes` on a fresh record ("" = served)"""
    hc = hostcheck_lib()
    hc.ba_hostcheck_guard.restype = ctypes.c_int
    ev = np.array([EVENTS.index(c) for c in codes], dtype=np.int32)
    msg = ctypes.create_string_buffer(512)
    rc = hc.ba_hostcheck_guard(ctypes.c_uint32(len(ev)), ev.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), guard.encode(),
                               who.encode(), noun.encode() if noun else None, ctypes.c_uint32(facts), ctypes.c_uint32(flags),
                               ctypes.c_double(lcs.PCG_TOL), ctypes.c_uint32(0), msg, ctypes.c_uint32(512))
    assert rc in (0, 1), (rc, guard)
    assert bool(rc) == bool(msg.value)
    return msg.value.decode()


def test_the_guards_decide_every_cell_as_the_rules_do():
    """Every cell of the event x reader matrix, and beyond it every prefix of every event's code sequence: the guard
    of requests.h that the reader's entry point asks serves exactly where the reader's rule serves, and where it
    refuses its message matches the rule's regular expression.  (The rules remain the statement the matrix of
    DESIGN.md is derived from; this holds the product code to them without a device.)"""
    import re
    cells = 0
    for ev in lcs.EVENT_LIST:
        t = lcs.Tracker(lcs.SETUPS[ev.setup])
        for r in lcs.READERS:
            t.expect(r)
        t.fire(*ev.codes)
        for r in lcs.READERS:
            codes = list(t.codes) + list(r.before_codes)      # what has fired when the reader's guard looks
            out, bits = t.expect(r)
            got = _ask_guard(codes, *_guard_of(r))
            assert (got == "") == (out[0] == "serve"), (ev.name, r.name, out, got)
            if got:
                assert re.search(out[2], got), (ev.name, r.name, out[2], got)
            cells += 1
        # every prefix of everything this engine has fired by now, for every reader and the calibration getter
        history = lcs.replay(*t.codes)
        for k in range(len(t.codes) + 1):
            bits = history[k - 1] if k else frozenset()
            for r in lcs.READERS + [lcs.CALIBRATION_READER]:
                out = r.rule(bits)
                got = _ask_guard(t.codes[:k], *_guard_of(r))
                assert (got == "") == (out[0] == "serve"), (ev.name, k, r.name, out, got)
                if got:
                    assert re.search(out[2], got), (ev.name, k, r.name, out[2], got)
    assert cells == len(lcs.EVENT_LIST) * len(lcs.READERS) == 437


def test_the_guards_read_the_engine_facts():
    """the branches of the guards that no single-GPU engine reaches: sharded engines, the distributed solve, a system
    factorised in place, a PCG plan of another system, missing or unusable PCG options"""
    import re
    direct, pcg = lcs.SETUP, lcs.SETUP_PCG
    DIST, SHARDED, HOOKED = 1, 2, 4
    who = "ba_hip_get_joint_state_marginals"
    assert _ask_guard(direct, "kept_factor", who, "joint marginals", SHARDED, LANDMARKS) == \
        who + ": landmark blocks are not available on sharded engines (each rank holds one landmark shard)"
    assert _ask_guard(direct, "kept_factor", who, "joint marginals", SHARDED, 0) == ""
    assert _ask_guard(direct, "kept_factor", who, "joint marginals", SHARDED | DIST, LANDMARKS) == \
        who + ": not available with the distributed solve"
    assert _ask_guard(direct, "marginals", "w", None, DIST, 0) == "w: not available with the distributed solve"
    # the calibration getter's wording, and its later place for the distributed solve
    cal = "ba_hip_get_calibration_marginals"
    assert _ask_guard(direct, "kept_factor", cal, None, DIST, 0) == "calibration marginals: not available with the distributed solve"
    assert _ask_guard(lcs.UPLOAD + lcs.FINALIZE, "kept_factor", cal, None, DIST, 0) == cal + " needs the factor of the last ba_hip_solve_gn"
    assert _ask_guard((), "kept_factor", cal, None, 0, 0) == "ba_hip_finalize has not been called"
    foreign = direct + ("selinv_released", "standalone_factorisation")
    assert re.search(lcs.FOREIGN, _ask_guard(foreign, "kept_factor", "w", "weakest modes", 0, 0))
    assert _ask_guard(foreign, "kept_factor", "w", "weakest modes", 0, FOREIGN_OK) == ""
    # the reduced system
    assert _ask_guard(direct, "get_S", "", None, 0, 0).startswith("S was factorised in place")
    assert _ask_guard(direct, "get_S", "", None, KEPT_COPY, 0) == "" and _ask_guard(pcg, "get_S", "", None, 0, 0) == ""
    assert re.search(lcs.NO_CHECK, _ask_guard(direct, "check_solve", "", None, 0, 0))
    assert _ask_guard(pcg, "check_solve", "", None, 0, 0) == ""
    assert _ask_guard(pcg, "check_solve", "", None, SHARDED, 0) == "ba_hip_check_solve: single shard only"
    # panel PCG
    w = "ba_hip_pcg_panel_solve_system"
    assert _ask_guard(pcg, "pcg_panel", w, None, PLAN_FITS, HAS_OPTIONS) == ""
    assert _ask_guard(pcg, "pcg_panel", w, None, 0, HAS_OPTIONS) == w + ": the plan of the last PCG solve does not match the system"
    assert _ask_guard(pcg, "pcg_panel", w, None, PLAN_FITS, 0) == w + ": NULL argument"
    for facts in (HOOKED, DIST):
        assert _ask_guard((), "pcg_panel", w, None, facts | PLAN_FITS, HAS_OPTIONS) == \
            w + ": not available on a sharded engine (all-reduce hook, collectives hook or communicator set)"
    # marginalize and the coarse statistics
    assert _ask_guard(direct, "marginalize", "", None, 0, 0) == ""
    assert _ask_guard(direct, "marginalize", "", None, 0, 8) == "marginalize: not offered with calibration unknowns"
    assert _ask_guard(direct, "marginalize", "", None, HOOKED, 0) == "marginalize: not offered on sharded engines or with the distributed solve"
    coarse = lcs.UPLOAD + lcs.FINALIZE + ("gn_solve_begins", "pcg_run_begins", "pcg_run_finished_coarse", "solved_by_pcg")
    assert _ask_guard(coarse, "pcg_coarse_stats", "", None, 0, 0) == ""
    assert _ask_guard(pcg, "pcg_coarse_stats", "", None, 0, 0) == "ba_hip_get_pcg_coarse_stats: the last solve did not use the coarse space"
    hc = hostcheck_lib()
    hc.ba_hostcheck_guard.restype = ctypes.c_int
    bad = np.array([len(EVENTS)], dtype=np.int32)
    msg = ctypes.create_string_buffer(8)
    args = (b"w", None, ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_double(0.5), ctypes.c_uint32(0), msg, ctypes.c_uint32(8))
    assert hc.ba_hostcheck_guard(ctypes.c_uint32(1), bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), b"get_S", *args) == -1
    assert hc.ba_hostcheck_guard(ctypes.c_uint32(0), None, b"no_such_guard", *args) == -1000


# ---- states A and B are far enough apart (the oracle on the CPU) ------------------------------------------------
def _oracle_system(sc, pa, obs, poses, terms):
    import copy
    from oracle import pyoracle as po
    from helpers import gn_options
    import pplever_cases as pc
    ba = po.OracleBundleAdjuster(1, 6)
    ba.Init(gn_options(po, apply_results=0))
    ba.AddCamera(sc.cam_params)
    ba.add_poses(poses, is_active=pa)
    ba.add_landmarks(sc.landmarks, sc.lm_ref_pose)
    ba.add_projection_residuals(*obs)
    s2 = copy.copy(sc)
    s2.poses = poses
    pc.add_to_oracle(ba, s2, terms)
    ba.Solve(1)
    S = ba.S()
    S = np.where(S == 0.0, S.T, S)
    dz = pc.oracle_jacobians(ba, terms)[0]
    return S, ba.rhs(), dz, ba.proj_jacobians()


def test_states_are_separated():
    """The dense references of states A and B, from the oracle's S on the CPU: for the fixed perturbation SHIFT every
    reader's reference at B lies more than 100 tolerances from the one at A, in the reader's own error measure — a
    stale read of A's numbers cannot pass B's check.  (The device test asserts the same on the engine's numbers.)"""
    import leverage_cases as lc
    import pplever_cases as pc
    sc, pa, obs, poses_a, poses_b = lcs.scene_AB()
    terms = pc.helper_terms(sc, lcs.P)
    (Sa, ra, dza, ja), (Sb, rb, dzb, jb) = (_oracle_system(sc, pa, obs, p, terms) for p in (poses_a, poses_b))
    assert Sa.shape == Sb.shape == (72, 72)
    tol = max(lc.tolerance(Sa), lc.tolerance(Sb))
    cond = max(np.linalg.cond(Sa), np.linalg.cond(Sb))
    pcg_bound = cond * lcs.PCG_TOL + 4.5 * np.finfo(np.float64).eps * cond
    Ia, Ib = np.linalg.inv(Sa), np.linalg.inv(Sb)
    d = np.sqrt(np.diag(Ib))
    rows = lc.natural_rows(pa)
    rr = lambda ids: np.array([rows[p] + x for p in ids for x in range(6)])
    corr = lambda r, c: float((np.abs(Ia - Ib)[np.ix_(r, c)] / np.outer(d[r], d[c])).max())
    sep = {}
    sep["pose_marginals"] = min(corr(rr([p]), rr([p])) for p in lcs.POSE_IDS) / tol
    sep["pose_pair_marginals"] = min(corr(rr([a]), rr([b])) for a, b in zip(lcs.PAIR_A, lcs.PAIR_B)) / tol
    sep["joint_marginals"] = corr(rr(lcs.JOINT_IDS), rr(lcs.JOINT_IDS)) / tol
    Xa, Xb = Ia @ lcs.RHS, Ib @ lcs.RHS
    rel = float((np.linalg.norm(Xa - Xb, axis=0) / np.linalg.norm(Xb, axis=0)).min())
    sep["factor_solve"] = rel / tol
    sep["pcg_panel_solve_system"] = rel / pcg_bound
    r = rr(lcs.JOINT_IDS)
    sep["joint_marginals_pcg"] = np.linalg.norm((Ia - Ib)[np.ix_(r, r)], 2) / np.linalg.norm(Ib[np.ix_(r, r)], 2) / pcg_bound
    wa, wb = (np.sort(np.abs(np.linalg.eigvalsh(S)))[:lcs.MODES] for S in (Sa, Sb))
    sep["weakest_modes"] = float(np.max(np.abs(wa - wb) / wb)) / tol
    sep["get_S"] = float(np.abs(Sa - Sb).max() / np.abs(Sb).max()) / tol
    sep["check_solve"] = abs(np.linalg.norm(ra) - np.linalg.norm(rb)) / np.linalg.norm(rb) / tol
    # hat blocks of the pose-pose residuals, whitened with the information the engine starts from (unary scale 1)
    info, w = pc.informations(terms)
    lam = info * w[:, None, None]
    masks = np.zeros(lcs.P, dtype=np.uint16)
    G = pc.whitened_rows(terms, 6, dzb, lam, pa, masks)[2]
    R = pc.res_dim(terms, 6)
    ca, cb = pc.reference_cov(terms, 6, dza, pa, masks, Ia), pc.reference_cov(terms, 6, dzb, pa, masks, Ib)
    for kind, name in ((0, "pose_pose_leverages_unary"), (1, "pose_pose_leverages_binary")):
        sl = terms.kind_slice(kind)
        sep[name] = pc.block_err(pc.whiten(ca[sl], G[sl], R[sl]), pc.whiten(cb[sl], G[sl], R[sl])) / tol
    # hat blocks of the projection residuals and the landmark blocks, from the oracle's whitened Jacobians
    nres = len(obs[1])
    ids = [0, 7, nres // 2, nres - 1]
    la = np.ones(lcs.L, dtype=np.uint8)
    hat, lmk, jst = [], [], []
    for S, (jm, jr, jl) in ((Sa, ja), (Sb, jb)):
        assert len(jm) == nres
        J, n = lc.dense_jacobian(1, 6, 0, pa, la, sc.lm_ref_pose, obs[1], obs[2], jm, jr, jl)
        H = J.T @ J
        full = np.linalg.inv(np.block([[S + H[:n, n:] @ np.linalg.solve(H[n:, n:], H[n:, :n]), H[:n, n:]], [H[n:, :n], H[n:, n:]]]))
        rows2 = np.concatenate([[2 * a, 2 * a + 1] for a in ids])
        Ja = J[rows2]
        hat.append(np.stack([Ja[2 * q:2 * q + 2] @ full @ Ja[2 * q:2 * q + 2].T for q in range(len(ids))]))
        lmk.append(np.array([full[n + l, n + l] for l in lcs.LM_IDS]))
        sel = np.concatenate([rr(lcs.POSE_IDS), n + np.array(lcs.LM_IDS)])
        jst.append(full[np.ix_(sel, sel)])
    sep["projection_leverages"] = float(np.abs(hat[0] - hat[1]).max()) / tol
    sep["landmark_marginals"] = float((np.abs(lmk[0] - lmk[1]) / lmk[1]).min()) / tol
    dj = np.sqrt(np.diag(jst[1]))
    sep["joint_state_marginals"] = float((np.abs(jst[0] - jst[1]) / np.outer(dj, dj)).max()) / tol
    print("separation of state B from state A in tolerances (tol %.3g, cond %.3g): %s"
          % (tol, cond, {k: "%.3g" % v for k, v in sep.items()}))
    for name, v in sep.items():
        assert v > 100.0, (name, v)
