"""The engine's lifecycle record (ba_amd/csrc/lifecycle.h) on the CPU: ba_hostcheck_lifecycle replays a list of
events on a fresh record and returns the flags after each one.  The sequences below are the event table of DESIGN.md
("What the engine holds and what drops it") stated as a test."""
import ctypes

import numpy as np
import pytest

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
