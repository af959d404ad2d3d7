// What the entry points ask before they read held state: is it there (the guards), and which rows does the request
// name (the row selection and the small argument checks).  Pure functions of the lifecycle record, a few engine facts
// and a view of the structure; each returns an empty string or the message of the refusal, first refusal first.
// Host only: no HIP include, hostcheck.cpp applies the same functions (ba_hostcheck_guard, ba_hostcheck_selection).
// A new reader adds a line here, not a paragraph in the engine (DESIGN.md "The request layer").
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "lifecycle.h"
#include "none_row.h"
#include "structure.h"

namespace bae {

// ---- the guards ----------------------------------------------------------------------------------------------------
// the engine facts beside the record that a guard reads
struct GuardFacts {
  bool dist_solve;     // the distributed reduced solve is enabled
  bool sharded;        // the engine holds one landmark shard of several
  bool hooked;         // an all-reduce hook, a collectives hook or a communicator is set
  bool kept_copy;      // keep_reduced_system is set and A_keep holds a copy of S
  bool pcg_plan_fits;  // the plan of the last PCG solve has the tile count and row blocks of the system
  bool damped;         // the linearisation the device holds was built with lambda > 0 (ba_hip_set_damping)
};
// The kept factor, the factor rows and the S of a damped linearisation belong to H + lambda D: what would read a
// covariance, a leverage, a mode or a prior out of them refuses.  ba_hip_get_S and ba_hip_check_solve keep serving:
// they read the damped S, which is what ba_hip_solve_gn solved.
static const char* const kDamped =
    "the linearisation the device holds is damped (ba_hip_set_damping), linearise and solve once with damping 0";
static const char* const kNotFinalized = "ba_hip_finalize has not been called";

// Is the factor that the last ba_hip_solve_gn left in A there to be read?  `who` starts the message, `noun` names what
// was asked for.  foreign_ok: a stand-alone solve since then does not matter to the caller.  landmarks: the request
// reads landmark blocks.  ba_hip_get_calibration_marginals (noun == nullptr) is older than the rest and keeps its
// shorter wording, and its later place for the distributed solve.
inline std::string guard_kept_factor(const Held& h, const GuardFacts& f, const char* who, const char* noun, bool foreign_ok,
                                     bool landmarks = false) {
  const std::string w = who, m = noun ? w + ": " : std::string();
  if (!h.finalized) return m + kNotFinalized;
  if (landmarks && f.sharded && !f.dist_solve)   // (the distributed solve refuses first, for every block)
    return m + "landmark blocks are not available on sharded engines (each rank holds one landmark shard)";
  if (noun && f.dist_solve) return m + "not available with the distributed solve";
  if (noun && f.damped) return m + kDamped;   // (calibration marginals cannot meet damping: it refuses calibration unknowns)
  if (!h.factored && h.pcg_solved)
    return w + ": the last ba_hip_solve_gn ran the PCG solver (BA_HIP_SOLVER_PCG), which leaves no factor" +
           (noun ? std::string("; ") + noun + " need a direct solve (ba_hip_set_reduced_solver)" : "");
  if (!h.factored)
    return noun ? m + "needs the factor of the last ba_hip_solve_gn (none yet, or the system was re-linearised since)"
                : w + " needs the factor of the last ba_hip_solve_gn";
  if (h.factor_foreign && !foreign_ok)
    return w + ": a stand-alone solve (ba_hip_tile_solve / ba_hip_dense_solve) has replaced the kept factor "
               "since the last ba_hip_solve_gn";
  if (!noun && f.dist_solve) return "calibration marginals: not available with the distributed solve";
  return "";
}
// ... for what reads the selected inverse: one computed before a stand-alone solve stays good
inline std::string guard_marginals(const Held& h, const GuardFacts& f, const char* who, bool landmarks) {
  return guard_kept_factor(h, f, who, "marginals", h.sig_valid, landmarks);
}

// what a caller's ba_hip_pcg_options says, for the checks below (null where the caller passed none)
struct PcgAsk {
  double rel_tolerance;
  uint32_t coarse_aggregate;
};
// A panel solve has no coarse space.  The engine's panel readers refuse it before they look at the tolerance, the
// stand-alone ba_hip_pcg_panel_solve has always named the tolerance first.
enum PcgCoarse { kCoarseRefusedFirst, kCoarseAllowed, kCoarseRefusedLast };
inline std::string pcg_options_ok(const char* who, const PcgAsk& o, PcgCoarse coarse) {
  const std::string m = std::string(who) + ": ";
  const bool bad_tol = !(o.rel_tolerance > 0.0) || !(o.rel_tolerance < 1.0);
  if (coarse != kCoarseAllowed && o.coarse_aggregate && !(coarse == kCoarseRefusedLast && bad_tol))
    return m + "coarse_aggregate must be 0: the coarse space is not available in panel solves";
  if (bad_tol) return m + "rel_tolerance must lie in (0, 1)";
  return "";
}
// Panel PCG on the engine's system: A must still hold the S that the last ba_hip_solve_gn solved by PCG.
inline std::string guard_pcg_panel(const Held& h, const GuardFacts& f, const char* who, const PcgAsk* o) {
  const std::string m = std::string(who) + ": ";
  if (f.hooked || f.dist_solve) return m + "not available on a sharded engine (all-reduce hook, collectives hook or communicator set)";
  if (!h.finalized) return m + kNotFinalized;
  if (f.damped) return m + kDamped;
  if (!h.pcg_solved) {
    if (h.factored)
      return m + "the last ba_hip_solve_gn ran the direct solver, A holds its factor and not S; panel solves need "
                 "a PCG solve (ba_hip_set_reduced_solver, BA_HIP_SOLVER_PCG); ba_hip_factor_solve serves the factor";
    if (h.pcg_last) return m + "the system was re-linearised since the PCG solve of the last ba_hip_solve_gn";
    return m + "needs a PCG solve by the last ba_hip_solve_gn (BA_HIP_SOLVER_PCG; none yet, or the system was "
               "re-linearised since)";
  }
  if (!o) return m + "NULL argument";
  const std::string bad = pcg_options_ok(who, *o, kCoarseRefusedFirst);
  if (!bad.empty()) return bad;
  if (!f.pcg_plan_fits) return m + "the plan of the last PCG solve does not match the system";
  return "";
}
inline std::string guard_check_solve(const Held& h, const GuardFacts& f) {
  if (!h.finalized) return kNotFinalized;
  if (!h.pcg_solved && !(h.factored && f.kept_copy))   // (after a PCG solve A itself still holds S)
    return "ba_hip_check_solve needs keep_reduced_system and a finished ba_hip_solve_gn";
  if (f.sharded) return "ba_hip_check_solve: single shard only";
  return "";
}
inline std::string guard_get_S(const Held& h, const GuardFacts& f) {
  if (!h.finalized) return kNotFinalized;
  if (h.factored && !f.kept_copy) return "S was factorised in place; set keep_reduced_system to read it after ba_hip_solve_gn";
  return "";
}
inline std::string guard_pcg_stats(const Held& h) {
  return h.pcg_last ? "" : "ba_hip_get_pcg_stats: the last ba_hip_solve_gn did not run the PCG solver";
}
inline std::string guard_pcg_coarse_stats(const Held& h) {
  return h.pcg_coarse_last ? "" : "ba_hip_get_pcg_coarse_stats: the last solve did not use the coarse space";
}
inline std::string guard_marginalize(const Held& h, const GuardFacts& f, bool calibration) {
  if (!h.finalized) return kNotFinalized;
  if (calibration) return "marginalize: not offered with calibration unknowns";
  if (f.hooked) return "marginalize: not offered on sharded engines or with the distributed solve";
  if (f.damped) return std::string("marginalize: ") + kDamped;
  if (!h.lin_valid)
    return "marginalize: needs the linearisation of the current state (ba_hip_linearize, no step, rollback or "
           "new masks since)";
  return "";
}

// ba_hip_triangulate_landmarks: the engine facts first (in_solve: between ba_hip_begin_solve and ba_hip_end_solve, where
// x_w lags behind x_s), then what the caller's options say, then the ids (each below L, each once)
struct TriAsk {
  int max_iterations;
  double lambda0, gradient_tolerance, step_tolerance, min_parallax, huber_width;
};
inline std::string guard_triangulate(const Held& h, const GuardFacts& f, bool calibration, int lm_dim, bool in_solve) {
  static const std::string m = "ba_hip_triangulate_landmarks: ";
  if (!h.finalized) return m + kNotFinalized;
  if (lm_dim == 0) return m + "LmSize 0 has no landmark unknowns";
  if (calibration) return m + "not offered with calibration unknowns";
  if (f.hooked || f.sharded || f.dist_solve) return m + "not offered on sharded engines or with the distributed solve";
  if (in_solve)
    return m + "not offered inside a Solve, where x_w lags behind the state: call ba_hip_end_solve first (or triangulate "
               "before ba_hip_begin_solve)";
  return "";
}
inline std::string triangulation_ok(const TriAsk& o, uint32_t L, uint32_t n, const uint32_t* ids) {
  static const std::string m = "ba_hip_triangulate_landmarks: ";
  if (o.max_iterations < 0 || o.max_iterations > 64)
    return m + "max_iterations " + std::to_string(o.max_iterations) + " does not lie in 0 .. 64";
  // (written so that a NaN is refused too)
  if (!(o.lambda0 >= 0.0) || !(o.gradient_tolerance >= 0.0) || !(o.step_tolerance >= 0.0) || !(o.min_parallax >= 0.0) ||
      !(o.huber_width >= 0.0))
    return m + "lambda0, the tolerances, min_parallax and huber_width must not be negative";
  if (!ids) return n == L ? "" : m + "with NULL ids n must be the landmark count";
  std::vector<uint8_t> seen(L, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (ids[i] >= L) return m + "id " + std::to_string(ids[i]) + " is not a landmark (there are " + std::to_string(L) + ")";
    if (seen[ids[i]]) return m + "landmark " + std::to_string(ids[i]) + " is named twice";
    seen[ids[i]] = 1;
  }
  return "";
}

// ba_hip_refine_poses: the same order as ba_hip_triangulate_landmarks (in_solve: x_w lags behind x_s with LmSize 1, and
// the poses held are those of a step that may still be rolled back), then the options, then the ids
struct RefineAsk {
  int max_iterations;
  unsigned fixed_mask;
  double initial_damping, gradient_tolerance, step_tolerance, huber_width;
};
inline std::string guard_refine_poses(const Held& h, const GuardFacts& f, bool calibration, int lm_dim, bool in_solve) {
  static const std::string m = "ba_hip_refine_poses: ";
  if (!h.finalized) return m + kNotFinalized;
  if (lm_dim == 0) return m + "LmSize 0 has no landmarks to resect against";
  if (calibration) return m + "not offered with calibration unknowns";
  if (f.hooked || f.sharded || f.dist_solve) return m + "not offered on sharded engines or with the distributed solve";
  if (in_solve)
    return m + "not offered inside a Solve, where x_w lags behind the state: call ba_hip_end_solve first (or refine "
               "before ba_hip_begin_solve)";
  return "";
}
inline std::string refinement_ok(const RefineAsk& o, uint32_t P, uint32_t n, const uint32_t* ids) {
  static const std::string m = "ba_hip_refine_poses: ";
  if (o.max_iterations < 0 || o.max_iterations > 64)
    return m + "max_iterations " + std::to_string(o.max_iterations) + " does not lie in 0 .. 64";
  // (written so that a NaN is refused too)
  if (!(o.initial_damping >= 0.0) || !(o.gradient_tolerance >= 0.0) || !(o.step_tolerance >= 0.0) || !(o.huber_width >= 0.0))
    return m + "initial_damping, the tolerances and huber_width must not be negative";
  if (o.fixed_mask >= 63) return m + "fixed_mask " + std::to_string(o.fixed_mask) + " leaves no free parameter (bits 0 .. 5, not all)";
  if (n == 0) return m + "no pose requested";
  if (!ids) return n == P ? "" : m + "with NULL ids n must be the pose count";
  std::vector<uint8_t> seen(P, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (ids[i] >= P) return m + "id " + std::to_string(ids[i]) + " is not a pose (there are " + std::to_string(P) + ")";
    if (seen[ids[i]]) return m + "pose " + std::to_string(ids[i]) + " is named twice";
    seen[ids[i]] = 1;
  }
  return "";
}

// ---- the small shared checks ---------------------------------------------------------------------------------------
// with NULL ids a request means all `count` of them: `count_name` ends the message
inline std::string ids_or_all(const char* who, const void* ids, uint32_t n, uint32_t count, const std::string& count_name) {
  return !ids && n != count ? std::string(who) + ": with NULL ids n must be " + count_name : "";
}
inline std::string residual_id_ok(const char* who, uint32_t id, uint32_t count, const char* kind) {   // kind: "a unary", ...
  return id < count ? "" : std::string(who) + ": id " + std::to_string(id) + " is not " + kind + " residual (there are " +
                               std::to_string(count) + ")";
}
static const uint32_t kRequestMaxBlock = 16;   // kPcgMaxBlock of pcg.h (engine_readers.hip asserts it)
inline std::string block_ok(const char* who, uint32_t block) {
  return block < 1 || block > kRequestMaxBlock ? std::string(who) + ": block must lie in 1 .. 16" : "";
}
inline std::string columns_ok(const char* who, uint64_t m, uint64_t limit, const char* limit_name,
                              const char* nothing = "no columns requested (m == 0)") {
  const std::string w = std::string(who) + ": ";
  if (m == 0) return w + nothing;
  if (m > limit) return w + std::to_string(m) + " columns requested, the limit is " + limit_name + " (" + std::to_string(limit) + ")";
  return "";
}

// ---- rows ----------------------------------------------------------------------------------------------------------
// what the checks read of the structure that ba_hip_finalize built
struct StructureView {
  uint32_t P, L, np, K, n, ld, D, LM;
  const std::vector<int32_t>*pose_opt, *lm_opt;
  const std::vector<uint32_t>* opt_of_natural;   // the pose ordering (empty: identity)
};
// Public outputs are indexed by the NATURAL optimisation index: row r of the caller's numbering is row int_row(r) of
// the engine's (the pose ordering of ba_hip_set_pose_ordering; the calibration border stays last).
inline uint32_t int_row(const StructureView& v, uint32_t r) {
  if (v.opt_of_natural->empty() || r >= v.np) return r;
  return (*v.opt_of_natural)[r / v.D] * v.D + r % v.D;
}
// per row of the engine's padded system the caller's row, kNoneRow for padding: the engine's own system ...
inline std::vector<uint32_t> natural_rowmap(const StructureView& v) {
  std::vector<uint32_t> m(v.ld, kNoneRow);
  for (uint32_t r = 0; r < v.n; ++r) m[int_row(v, r)] = r;
  return m;
}
// ... and a stand-alone system of n rows padded to ld
inline std::vector<uint32_t> identity_rowmap(uint32_t n, uint32_t ld) {
  std::vector<uint32_t> m(ld, kNoneRow);
  for (uint32_t r = 0; r < n; ++r) m[r] = r;
  return m;
}
// first row of an active pose's block in the engine's numbering
inline std::string pose_row(const StructureView& v, const char* who, uint32_t id, uint32_t* row) {
  if (id >= v.P || (*v.pose_opt)[id] < 0)
    return std::string(who) + ": pose " + std::to_string(id) + " is not an active pose (it has no columns in S)";
  *row = (uint32_t)(*v.pose_opt)[id] * v.D;
  return "";
}
inline std::string landmark_active(const StructureView& v, const char* who, uint32_t id) {
  return id >= v.L || (*v.lm_opt)[id] < 0 ? std::string(who) + ": landmark " + std::to_string(id) + " is not an active landmark" : "";
}
inline std::string not_repeated(const char* who, const char* what, const uint32_t* ids, uint32_t n) {
  std::vector<uint32_t> seen(ids, ids + n);
  std::sort(seen.begin(), seen.end());
  for (uint32_t i = 0; i + 1 < n; ++i)
    if (seen[i] == seen[i + 1])
      return std::string(who) + ": " + what + " " + std::to_string(seen[i]) + " is repeated (the joint block would be singular)";
  return "";
}

// A joint request: the D rows of every pose in request order, then the K calibration rows, then the landmarks' columns.
struct RowRequest {
  const char* who;
  uint32_t n_poses;
  const uint32_t* pose_ids;
  bool include_calibration;
  uint32_t n_lms;
  const uint32_t* lm_ids;
  bool have_out;            // the caller passed an output buffer
  uint64_t limit;           // most columns of one request, and the name of that limit
  const char* limit_name;
  const char* nothing;      // the wording when the request names no column
  bool caller_numbering;    // rows in the caller's numbering (what the panel solves take), not the engine's
};
struct RowSelection {
  std::vector<uint32_t> rows, lms;
};
inline std::string select_rows(const StructureView& v, const RowRequest& q, RowSelection* out) {
  const std::string m = std::string(q.who) + ": ";
  if ((q.n_poses && !q.pose_ids) || (q.n_lms && !q.lm_ids) || !q.have_out) return m + "NULL argument";
  if (q.include_calibration && !v.K) return m + "include_calibration without calibration unknowns (ba_hip_set_calibration)";
  const uint64_t M = (uint64_t)q.n_poses * v.D + (q.include_calibration ? v.K : 0) + (uint64_t)q.n_lms * v.LM;
  // (the panel getter has always counted in 32 bits: its message says so past 2^32 columns)
  std::string bad = columns_ok(q.who, q.caller_numbering && M > 0xffffffffu ? 0xffffffffu : M, q.limit, q.limit_name, q.nothing);
  if (bad.empty()) bad = not_repeated(q.who, "pose", q.pose_ids, q.n_poses);
  if (!bad.empty()) return bad;
  std::vector<uint32_t> nat_of_int;
  if (q.caller_numbering) nat_of_int = natural_rowmap(v);
  out->rows.clear();
  out->rows.reserve(M);
  for (uint32_t i = 0; i < q.n_poses; ++i) {
    uint32_t r = 0;
    if (!(bad = pose_row(v, q.who, q.pose_ids[i], &r)).empty()) return bad;
    for (uint32_t x = 0; x < v.D; ++x) out->rows.push_back(q.caller_numbering ? nat_of_int[r + x] : r + x);
  }
  if (q.include_calibration)
    for (uint32_t x = 0; x < v.K; ++x) out->rows.push_back(v.np + x);
  out->lms.assign(q.lm_ids, q.lm_ids + q.n_lms);
  if (!(bad = not_repeated(q.who, "landmark", q.lm_ids, q.n_lms)).empty()) return bad;
  for (uint32_t id : out->lms)
    if (!(bad = landmark_active(v, q.who, id)).empty()) return bad;
  return "";
}

}  // namespace bae
