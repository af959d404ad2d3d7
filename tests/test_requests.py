"""The request layer (ba_amd/csrc/requests.h) on the CPU, through the taps of hostcheck.cpp: the row selection of the
joint getters on one hand-made structure, the small shared checks at their edges, the two row maps, and a source check
of how the entry points of engine.hip / engine_readers.hip begin.

The structure: 5 poses of which pose 1 is inactive, 4 landmarks of which landmark 2 is inactive, PoseSize 6 or 15, 0 or 6
calibration unknowns, LmSize 0, 1 or 3, natural order or the pose ordering [2, 0, 3, 1].  Expected rows come from
numpy.  Every refusal is matched with the regular expression the device tests use for it (test_joint_marginals_gpu.py,
test_joint_state_gpu.py, test_pcg_panel_gpu.py, test_marginals_gpu.py, test_leverages_gpu.py,
test_pose_pose_leverages_gpu.py).

With PoseSize 6 or 15 and 0 or 6 calibration rows a request without landmarks cannot name 512 or 513 columns: the panel
getter's limit is crossed at 516, and columns_ok itself is checked at 512 and 513."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from helpers import hostcheck_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xffffffff
JOINT_MAX = PANEL_MAX = 512      # BA_HIP_JOINT_MAX_COLUMNS, BA_HIP_PCG_PANEL_MAX_COLUMNS (include/ba_hip.h)
P, L = 5, 4
POSE_ACTIVE = np.array([1, 0, 1, 1, 1], dtype=bool)
LM_ACTIVE = np.array([1, 1, 0, 1], dtype=bool)
PERM = [2, 0, 3, 1]

# the wording of the device tests
NOT_ACTIVE_POSE = "is not an active pose"
NOT_ACTIVE_LM = "is not an active landmark"
REPEATED = "is repeated"
INCLUDE_CALIBRATION = "include_calibration"
NO_POSE = "no pose"
M_ZERO = "m == 0"
NULL = "NULL"
OVER_JOINT = "513 columns requested, the limit is BA_HIP_JOINT_MAX_COLUMNS \\(512\\)"
OVER_PANEL_ANY = "the limit is BA_HIP_PCG_PANEL_MAX_COLUMNS"
OVER_PANEL = "513 columns requested, the limit is BA_HIP_PCG_PANEL_MAX_COLUMNS \\(512\\)"


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


def _ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t)) if a is not None else None


def _header_limits():
    txt = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (BA_HIP_\w+_MAX_COLUMNS) (\d+)", txt)}


def test_the_limits_are_the_headers():
    lim = _header_limits()
    assert lim["BA_HIP_JOINT_MAX_COLUMNS"] == JOINT_MAX and lim["BA_HIP_PCG_PANEL_MAX_COLUMNS"] == PANEL_MAX


class Structure:
    def __init__(self, D, K, LM, perm):
        self.D, self.K, self.LM, self.perm = D, K, LM, list(perm)
        self.nat = np.full(P, -1, dtype=np.int32)          # natural optimisation index of every pose
        self.nat[POSE_ACTIVE] = np.arange(POSE_ACTIVE.sum())
        self.pose_opt = self.nat.copy()
        if perm:
            self.pose_opt[POSE_ACTIVE] = np.asarray(perm, dtype=np.int32)[self.nat[POSE_ACTIVE]]
        self.lm_opt = np.full(L, -1, dtype=np.int32)
        if LM:
            self.lm_opt[LM_ACTIVE] = np.arange(LM_ACTIVE.sum())
        self.np_ = int(POSE_ACTIVE.sum()) * D
        self.n = self.np_ + K
        self.ld = max(64, (self.n + 63) // 64 * 64)

    def int_row(self, r):
        if not self.perm or r >= self.np_:
            return r
        return self.perm[r // self.D] * self.D + r % self.D

    def expected_rows(self, poses, calibration, caller):
        rows = [int(self.pose_opt[p]) * self.D + x for p in poses for x in range(self.D)]
        rows += [self.np_ + x for x in range(self.K if calibration else 0)]
        if caller:
            inverse = {self.int_row(r): r for r in range(self.n)}
            rows = [inverse[r] for r in rows]
        return rows

    def select(self, poses, lms=(), calibration=False, caller=False, who="who", limit=JOINT_MAX,
               limit_name="BA_HIP_JOINT_MAX_COLUMNS", nothing="no pose and no calibration rows requested", have_out=True,
               null_poses=False, null_lms=False, n_poses=None, n_lms=None):
        """(rows, lms) of an accepted request, or the message of the refusal"""
        hc = hostcheck_lib()
        hc.ba_hostcheck_selection.restype = ctypes.c_int
        pid, lid, perm = _u32(list(poses)), _u32(list(lms)), _u32(self.perm)
        n_poses = len(pid) if n_poses is None else n_poses
        n_lms = len(lid) if n_lms is None else n_lms
        rows = np.full(n_poses * self.D + self.K + n_lms * max(self.LM, 1) + 1, NONE, dtype=np.uint32)
        out_lms = np.full(n_lms + 1, NONE, dtype=np.uint32)
        counts = np.zeros(2, dtype=np.uint32)
        msg = ctypes.create_string_buffer(512)
        U32 = ctypes.c_uint32
        rc = hc.ba_hostcheck_selection(
            U32(P), _ptr(self.pose_opt, ctypes.c_int32), U32(L), _ptr(self.lm_opt, ctypes.c_int32), U32(self.np_), U32(self.K),
            U32(self.D), U32(self.LM), U32(self.ld), U32(len(perm)), _ptr(perm, U32), who.encode(), U32(n_poses),
            None if null_poses else _ptr(pid, U32), ctypes.c_int(int(calibration)), U32(n_lms),
            None if null_lms else _ptr(lid, U32), ctypes.c_int(int(have_out)), ctypes.c_uint64(limit), limit_name.encode(),
            nothing.encode(), ctypes.c_int(int(caller)), _ptr(rows, U32), _ptr(out_lms, U32), _ptr(counts, U32), msg, U32(512))
        assert rc in (0, 1), rc
        if rc:
            assert msg.value
            return msg.value.decode()
        return [int(v) for v in rows[:counts[0]]], [int(v) for v in out_lms[:counts[1]]]

    def panel(self, poses, **kw):
        return self.select(poses, caller=True, limit=PANEL_MAX, limit_name="BA_HIP_PCG_PANEL_MAX_COLUMNS",
                           nothing="no columns requested (m == 0)", **kw)


STRUCTURES = [Structure(D, K, LM, perm) for D, K, LM, perm in itertools.product((6, 15), (0, 6), (0, 1, 3), ([], PERM))]
IDS = ["D%d-K%d-LM%d-%s" % (s.D, s.K, s.LM, "perm" if s.perm else "natural") for s in STRUCTURES]


def refused(got, pattern, who="who"):
    assert isinstance(got, str), "served: %r" % (got,)
    assert got.startswith(who + ": ") and re.search(pattern, got), (got, pattern)


@pytest.mark.parametrize("s", STRUCTURES, ids=IDS)
def test_accepted_selections_keep_the_request_order(s):
    lms = [3, 0] if s.LM else []
    for poses in ([4, 0, 3], [2], [3, 2, 0, 4], []):
        for cal in ([False, True] if s.K else [False]):
            for caller in (False, True):
                if not poses and not cal and (caller or not lms):
                    continue      # (names no column: test_refusals)
                got = s.select(poses, [] if caller else lms, cal, caller)
                assert got == (s.expected_rows(poses, cal, caller), [] if caller else lms), (poses, cal, caller)
    # n = 0 with NULL id pointers
    if s.K:
        assert s.select([], calibration=True, null_poses=True, null_lms=True) == (s.expected_rows([], True, False), [])
    # the ordering moves rows in the engine's numbering and none in the caller's
    nat = Structure(s.D, s.K, s.LM, [])
    assert s.select([4, 0], caller=True)[0] == nat.select([4, 0])[0]
    assert (s.select([4, 0])[0] != nat.select([4, 0])[0]) == bool(s.perm)


@pytest.mark.parametrize("s", STRUCTURES, ids=IDS)
def test_refusals(s):
    for sel, who in ((s.select, "ba_hip_get_joint_state_marginals"), (s.panel, "ba_hip_get_joint_marginals_pcg")):
        refused(sel([0, 3, 0], who=who), REPEATED, who)
        refused(sel([0, 3, 0], who=who), "pose 0 is repeated", who)
        refused(sel([0, 1], who=who), NOT_ACTIVE_POSE, who)
        refused(sel([P], who=who), NOT_ACTIVE_POSE, who)
        refused(sel([P + 3, 0], who=who), "pose %d is not an active pose" % (P + 3), who)
        refused(sel([0], who=who, null_poses=True), NULL, who)
        refused(sel([0], who=who, have_out=False), NULL, who)
        if not s.K:
            refused(sel([0], calibration=True, who=who), INCLUDE_CALIBRATION, who)
    # nothing requested, in both wordings
    refused(s.select([]), NO_POSE)
    refused(s.select([], nothing="no pose, no calibration rows and no landmark requested"), NO_POSE)
    refused(s.panel([]), M_ZERO)
    # a repeated pose is reported before an inactive one, an inactive pose before any landmark
    refused(s.select([1, 0, 0]), REPEATED)
    refused(s.select([1], [2, 2]), NOT_ACTIVE_POSE)
    # landmarks
    refused(s.select([0], [0], null_lms=True), NULL)
    if s.LM:
        refused(s.select([0], [3, 0, 3]), "landmark 3 is repeated")
        refused(s.select([0], [2]), "landmark 2 is not an active landmark")
        refused(s.select([0], [L]), NOT_ACTIVE_LM)
        refused(s.select([0], [2, 2]), REPEATED)        # repeated before inactive
    else:
        refused(s.select([0], [0]), NOT_ACTIVE_LM)    # LmSize 0: no landmark has columns
        refused(s.select([], [0]), NO_POSE)           # ... and a request of landmarks alone names no column


@pytest.mark.parametrize("s", STRUCTURES, ids=IDS)
def test_column_limits(s):
    """the column count is checked before the ids are looked at: repeated ids reach the limits on five poses"""
    per = s.D
    under = (JOINT_MAX - (s.K or 0)) // per            # the most poses that fit beside the calibration rows
    cal = bool(s.K)
    M = under * per + s.K
    assert M <= JOINT_MAX < M + per
    refused(s.select([0] * under, calibration=cal), REPEATED)                      # within the limit: the next check speaks
    over = s.select([0] * (under + 1), calibration=cal)
    refused(over, "%d columns requested, the limit is BA_HIP_JOINT_MAX_COLUMNS \\(512\\)" % (M + per))
    refused(s.panel([0] * under, calibration=cal), REPEATED)
    refused(s.panel([0] * (under + 1), calibration=cal), OVER_PANEL_ANY)
    refused(s.panel([0] * (under + 1), calibration=cal), "%d columns requested" % (M + per))
    if s.LM and (JOINT_MAX - M) % s.LM == 0:
        fill = (JOINT_MAX - M) // s.LM                 # landmarks up to exactly 512 columns, then one column over
        refused(s.select([0] * under, [0] * fill, calibration=cal), REPEATED)
        if s.LM == 1:
            refused(s.select([0] * under, [0] * (fill + 1), calibration=cal), OVER_JOINT)
    if s.D == 6 and s.LM == 3 and not s.K:
        refused(s.select([0] * 85, [0]), OVER_JOINT)   # 85 * 6 + 3 = 513


# ---- the small checks ----------------------------------------------------------------------------------------------
def check(op, who="who", name="", u=(), d=()):
    hc = hostcheck_lib()
    hc.ba_hostcheck_request_check.restype = ctypes.c_int
    ua = np.array(list(u) + [0], dtype=np.uint64)
    da = np.array(list(d) + [0.0], dtype=np.float64)
    msg = ctypes.create_string_buffer(512)
    rc = hc.ba_hostcheck_request_check(ctypes.c_int(op), who.encode(), name.encode(), _ptr(ua, ctypes.c_uint64),
                                       _ptr(da, ctypes.c_double), msg, ctypes.c_uint32(512))
    assert rc in (0, 1), rc
    assert bool(rc) == bool(msg.value)
    return msg.value.decode()


def test_ids_or_all():
    for have_ids, n, count, ok in ((0, 7, 7, True), (0, 0, 0, True), (0, 6, 7, False), (0, 8, 7, False), (0, 0, 7, False),
                                   (0, 1, 0, False), (1, 3, 7, True), (1, 0, 7, True), (1, 9, 7, True)):
        got = check(0, "ba_hip_get_projection_leverages", "the projection residual count", (have_ids, n, count))
        assert (got == "") == ok, (have_ids, n, count, got)
    assert re.search("n must be the projection residual count", check(0, "w", "the projection residual count", (0, 1, 2)))
    assert re.search("ba_hip_get_pose_pose_leverages: with NULL ids n must be the residual count",
                     check(0, "ba_hip_get_pose_pose_leverages", "the residual count of the kind (2)", (0, 1, 2)))
    assert check(0, "ba_hip_get_landmark_marginals", "the active landmark count", (0, 1, 2)) == \
        "ba_hip_get_landmark_marginals: with NULL ids n must be the active landmark count"


def test_pcg_options_ok():
    tiny = np.nextafter(0.0, 1.0)
    for tol, ok in ((0.0, False), (1.0, False), (float("nan"), False), (-1e-3, False), (float("inf"), False), (tiny, True),
                    (np.nextafter(1.0, 0.0), True), (1e-6, True)):
        for allow in (0, 1, 2):
            got = check(1, "ba_hip_pcg_solve", u=(0, allow), d=(tol,))
            assert (got == "") == ok, (tol, allow, got)
            if not ok:
                assert re.search("rel_tolerance", got) and got == "ba_hip_pcg_solve: rel_tolerance must lie in (0, 1)"
    # the coarse space: refused in panel solves, and before the tolerance
    assert check(1, u=(1, 1), d=(1e-6,)) == "" and check(1, u=(4, 1), d=(1e-6,)) == ""
    for tol in (1e-6, 0.0, float("nan")):
        assert re.search("coarse_aggregate must be 0", check(1, u=(1, 0), d=(tol,)))
    # ba_hip_pcg_panel_solve (mode 2) names the tolerance first, then the coarse space
    assert re.search("coarse_aggregate must be 0", check(1, "ba_hip_pcg_panel_solve", u=(1, 2), d=(1e-6,)))
    for tol in (0.0, 1.0, float("nan")):
        assert check(1, "ba_hip_pcg_panel_solve", u=(1, 2), d=(tol,)) == "ba_hip_pcg_panel_solve: rel_tolerance must lie in (0, 1)"
    assert check(1, u=(0, 2), d=(1e-6,)) == ""


def test_block_ok():
    for block, ok in ((0, False), (1, True), (15, True), (16, True), (17, False), (NONE, False)):
        got = check(2, "ba_hip_pcg_solve", u=(block,))
        assert (got == "") == ok, (block, got)
        if not ok:
            assert got == "ba_hip_pcg_solve: block must lie in 1 .. 16"


def test_columns_ok():
    name = "BA_HIP_PCG_PANEL_MAX_COLUMNS"
    assert re.search(M_ZERO, check(3, name=name, u=(0, PANEL_MAX)))
    for m in (1, PANEL_MAX - 1, PANEL_MAX):
        assert check(3, name=name, u=(m, PANEL_MAX)) == "", m
    assert re.search(OVER_PANEL, check(3, name=name, u=(PANEL_MAX + 1, PANEL_MAX)))
    assert re.search(OVER_JOINT, check(3, name="BA_HIP_JOINT_MAX_COLUMNS", u=(JOINT_MAX + 1, JOINT_MAX)))
    assert re.search("513 columns requested", check(3, name=name, u=(PANEL_MAX + 1, PANEL_MAX)))
    assert re.search("4294967296 columns requested", check(3, name=name, u=(1 << 32, PANEL_MAX)))


@pytest.mark.parametrize("s", STRUCTURES[::3], ids=IDS[::3])
def test_rowmaps(s):
    hc = hostcheck_lib()
    perm = _u32(s.perm)
    nat = np.zeros(s.ld, dtype=np.uint32)
    ident = np.zeros(s.ld, dtype=np.uint32)
    U32 = ctypes.c_uint32
    hc.ba_hostcheck_rowmaps(U32(s.np_), U32(s.K), U32(s.D), U32(s.ld), U32(len(perm)), _ptr(perm, U32), _ptr(nat, U32),
                            _ptr(ident, U32))
    want = np.full(s.ld, NONE, dtype=np.uint32)
    for r in range(s.n):
        want[s.int_row(r)] = r
    assert np.array_equal(nat, want)
    assert sorted(nat[nat != NONE]) == list(range(s.n)) and np.all(nat[s.n:] == NONE)   # the border stays last
    assert np.array_equal(ident, np.concatenate([np.arange(s.n), np.full(s.ld - s.n, NONE)]).astype(np.uint32))
    assert np.array_equal(nat, ident) == (not s.perm)


# ---- how the entry points begin (the sources) --------------------------------------------------------------------------
ENTRY_FILES = ("engine.hip", "engine_readers.hip")
UNGUARDED = {"ba_hip_create", "ba_hip_destroy", "ba_hip_last_error", "ba_hip_device_bytes_live", "ba_hip_lie",
             "ba_hip_dist_plan_stats", "ba_hip_solve_is_distributed",
             # the host-side inertial integration: no engine
             "ba_hip_integrate_imu", "ba_hip_integrate_imu_jacobians", "ba_hip_imu_pose_derivative", "ba_hip_imu_integrate_pose"}
GUARDS = ("BA_ENTRY_HOST(h);", "BA_ENTRY_DEVICE(h);", "BA_ENTRY_FINAL(h);")


def _source(name):
    with open(os.path.join(ROOT, "ba_amd", "csrc", name), encoding="utf-8") as f:
        return f.read()


def _definitions(txt):
    """(name, takes a const engine, body) of every ba_hip_* function defined at the top level of a source"""
    out = []
    for m in re.finditer(r"^[A-Za-z_][\w \*]*?\b(ba_hip_\w+)\(([^)]*)\)\s*\{", txt, flags=re.M):
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(txt[i], 0)
            i += 1
        out.append((m.group(1), "const ba_hip_engine*" in m.group(2), txt[m.end():i - 1]))
    return out


def test_every_entry_point_begins_with_a_guard():
    seen = set()
    for name in ENTRY_FILES:
        for fn, const_engine, body in _definitions(_source(name)):
            seen.add(fn)
            first = body.strip().split("\n")[0].strip()
            if fn in UNGUARDED or const_engine:      # (the counters on a const engine are one expression)
                assert not any(g in body for g in GUARDS), fn
            else:
                assert first in GUARDS, (name, fn, first)
    from ba_amd import hipapi
    assert len(seen) > 100
    missing = set(hipapi.SYMBOLS) - seen - {s for s in hipapi.SYMBOLS if s.startswith("ba_hip_comm_")}
    assert not missing, missing     # every other symbol of the header is defined in these two files


def test_the_device_is_selected_by_the_guard_alone():
    for name in ENTRY_FILES:
        for fn, _, body in _definitions(_source(name)):
            assert ("hipSetDevice" in body) == (fn in ("ba_hip_create", "ba_hip_destroy")), fn
        assert _source(name).count("hipSetDevice") == (2 if name == "engine.hip" else 0), name
    assert _source("entry.h").count("hipSetDevice(e->device)") == 2     # the two device forms


def test_the_deferred_sums_end_through_their_scope():
    for name in ENTRY_FILES:
        txt = _source(name)
        assert "defer_flush" not in txt and "defer_begin" not in txt, name
        assert "defer_active" not in txt and "defer_n" not in txt, name
    assert _source("engine.hip").count("DeferScope sums(e);") == 4
    assert _source("engine.h").count("defer_flush(e)") == 1
