// What the engine holds on the device that was derived from something else, and what drops it.
// One record (Engine::held), one method per event; the body of an event lists what it drops or establishes and
// why.  Nothing else assigns these flags (DESIGN.md "What the engine holds and what drops it").  Host only: no HIP
// include, hostcheck.cpp replays event lists on a fresh record (ba_hostcheck_lifecycle).
// The version counters (sig_plan_version, pcg_plan_version, tile_order_version, dist.key, bulk_lists.key,
// nzL_version) compare against each other and are a different mechanism: they stay on the engine.
#pragma once

namespace bae {

struct Held {
  bool finalized = false;        // the structure on the device belongs to the problem data as last set
  bool has_snapshot = false;     // buffer 1 - cur holds the state before the last applied step
  // err_cache: |r|^2 * original weight per observation at the state held in buffer 0 / 1, left behind by the last
  // EvaluateResiduals at that state; invalidated by everything that changes a state buffer or the cameras
  bool obs_e_valid[2] = {false, false};
  bool lin_valid = false;        // the device holds the last linearisation at the current state (ba_hip_marginalize)
  bool dog_jrhs_valid = false;   // dog_h[6], dog_h[7] (|J rhs|^2: projection / pose-pose part) belong to the current linearisation
  bool factored = false;         // A currently holds the Cholesky factor, not S
  bool factor_foreign = false;   // invdiag holds the factor of a stand-alone solve, not of A
  bool pcg_solved = false;       // the last ba_hip_solve_gn ran PCG and no linearisation since: gn_p solves the S in A
  bool pcg_last = false;         // the last ba_hip_solve_gn ran PCG (its statistics are host copies)
  bool pcg_coarse_last = false;  // the last solve (ba_hip_solve_gn or ba_hip_pcg_solve) used the coarse space
  bool sig_valid = false;        // sig (the selected inverse) belongs to the factor currently in A
  bool nzL_valid = false;        // nzL / nzL_host / nzS_host: the tile pattern of the factor of this structure and sharding
  bool marg_valid = false;       // marg_ids / marg_x0 / marg_H / marg_b / marg_c: a finished marginalisation (host copies)
  const void* A_cleared = nullptr;  // the allocation of A whose whole square has been zeroed once

  // ---- problem data and structure (ba_hip_set_*, ba_hip_finalize) ----
  void problem_changed() {
    finalized = false;           // part of the graph: takes effect at the next ba_hip_finalize
  }
  void calibration_changed() {
    problem_changed();
    dog_jrhs_valid = false;      // the calibration part of the sum appears or disappears
  }
  void pose_cam_params_changed() {
    drop_err_caches();           // uploaded without a rebuild: the residuals change
  }
  void finalize_begins() {
    finalized = false;           // a finalize that fails midway leaves the engine unfinalised
    dog_jrhs_valid = false;      // the factor rows are rebuilt: no cached sum survives
    drop_err_caches();           // the state buffers are re-uploaded
    lin_valid = false;           // ... and the rows of the last linearisation are gone
    factored = false;            // A is re-allocated for the new system: the factor, the PCG solution and the
    pcg_solved = false;          //   selected inverse of the old one must not be read with the new tile count.
    sig_valid = false;           //   (factor_foreign, pcg_last / pcg_coarse_last, marg_valid: host copies or facts
                                 //   about the last solve, they keep their values)
  }
  void structure_rebuilt() {
    nzL_valid = false;           // new tile pattern of S
    has_snapshot = false;        // the state starts again in buffer 0
    A_cleared = nullptr;         // new structure (possibly a new allocation / leading dimension): clear the square once
  }
  void finalize_succeeded() { finalized = true; }
  void sharding_changed() {      // ba_hip_set_allreduce, ba_hip_comm_init, ba_hip_comm_destroy
    nzL_valid = false;           // the tile pattern of S is the union over the shards
    dog_jrhs_valid = false;      // a local sum may have become a cross-shard one
  }
  void pattern_built() { nzL_valid = true; }   // factor_tile_pattern

  // ---- one Solve() ----
  void solve_begins() {          // ba_hip_begin_solve
    dog_jrhs_valid = false;
    drop_err_caches();           // x_s is re-derived from x_w, the cameras may have been re-uploaded
    lin_valid = false;
  }
  void masks_changed() {         // ba_hip_set_pose_masks; the factor in A is that of the old masks and stays readable
    dog_jrhs_valid = false;
    lin_valid = false;
  }
  void linearize_begins() {
    dog_jrhs_valid = false;      // the rows it was summed over are about to be rewritten
  }
  void linearize_writes_A() {    // before launch_gather_S; an error return before this point keeps the factor
    factored = false;            // A holds S again
    pcg_solved = false;          // ... of another linearisation than gn_p solves
    sig_valid = false;
    lin_valid = false;           // until the whole of it is there (linearize_succeeded)
  }
  void linearize_succeeded() { lin_valid = true; }
  void gn_solve_begins() {       // ba_hip_solve_gn
    sig_valid = false;           // the factor is about to be replaced
    pcg_last = pcg_solved = pcg_coarse_last = false;
  }
  void solved_by_pcg() {
    factored = false;            // S stays in A: no factor, no kept copy
    pcg_last = pcg_solved = true;
  }
  void solved_directly() {
    factored = true;
    factor_foreign = false;      // invdiag holds the factor of A again
  }
  void standalone_factorisation() {   // ba_hip_dense_solve, ba_hip_tile_solve
    factor_foreign = true;       // invdiag is about to hold this system's factor, not the scene's
  }
  void pcg_run_begins() { pcg_coarse_last = false; }               // pcg_solve_device
  void pcg_run_finished(bool coarse) { pcg_coarse_last = coarse; }
  void dogleg_sums(bool ok) { dog_jrhs_valid = ok; }               // ba_hip_dogleg_terms
  void step_applied(int new_cur) {
    has_snapshot = true;
    lin_valid = false;
    obs_e_valid[new_cur] = false;   // a new state in this buffer: no evaluation of it yet
  }
  void rolled_back() {
    has_snapshot = false;
    lin_valid = false;
  }
  void residuals_evaluated(int cur) { obs_e_valid[cur] = true; }   // launch_residuals mode 1

  // ---- results computed on request ----
  void selinv_computed() { sig_valid = true; }
  void selinv_released() { sig_valid = false; }
  void marginalize_failed() { marg_valid = false; }   // the store may hold a partial result
  void marginalized() { marg_valid = true; }
  void marginalization_released() { marg_valid = false; }
  void square_cleared(const void* A) { A_cleared = A; }   // launch_gather_S zeroed the whole square of this allocation
  void square_dirty() { A_cleared = nullptr; }            // debug key 3: other tiles get written from now on

  void drop_err_caches() { obs_e_valid[0] = obs_e_valid[1] = false; }
};

// ---- replay on a fresh record (hostcheck.cpp, tests/test_lifecycle.py): event codes and the bit order of the result
enum HeldBit {
  kHeldFinalized, kHeldSnapshot, kHeldErr0, kHeldErr1, kHeldLin, kHeldDogJrhs, kHeldFactored, kHeldForeign,
  kHeldPcgSolved, kHeldPcgLast, kHeldPcgCoarseLast, kHeldSig, kHeldPattern, kHeldMarg, kHeldSquareCleared
};
enum HeldEvent {
  kEvProblemChanged, kEvCalibrationChanged, kEvPoseCamParamsChanged, kEvFinalizeBegins, kEvStructureRebuilt,
  kEvFinalizeSucceeded, kEvShardingChanged, kEvPatternBuilt, kEvSolveBegins, kEvMasksChanged, kEvLinearizeBegins,
  kEvLinearizeWritesA, kEvLinearizeSucceeded, kEvGnSolveBegins, kEvSolvedByPcg, kEvSolvedDirectly,
  kEvStandaloneFactorisation, kEvPcgRunBegins, kEvPcgRunFinishedPlain, kEvPcgRunFinishedCoarse, kEvDoglegSumsOk,
  kEvDoglegSumsFailed, kEvStepAppliedTo0, kEvStepAppliedTo1, kEvRolledBack, kEvResidualsEvaluatedAt0,
  kEvResidualsEvaluatedAt1, kEvSelinvComputed, kEvSelinvReleased, kEvMarginalizeFailed, kEvMarginalized,
  kEvMarginalizationReleased, kEvSquareCleared, kEvSquareDirty, kEvCount
};

inline unsigned held_bits(const Held& h) {
  const bool b[] = {h.finalized, h.has_snapshot, h.obs_e_valid[0], h.obs_e_valid[1], h.lin_valid, h.dog_jrhs_valid,
                    h.factored, h.factor_foreign, h.pcg_solved, h.pcg_last, h.pcg_coarse_last, h.sig_valid,
                    h.nzL_valid, h.marg_valid, h.A_cleared != nullptr};
  unsigned v = 0;
  for (unsigned i = 0; i < sizeof(b) / sizeof(b[0]); ++i) v |= (b[i] ? 1u : 0u) << i;
  return v;
}

inline bool held_apply(Held& h, int event) {
  switch (event) {
    case kEvProblemChanged: h.problem_changed(); break;
    case kEvCalibrationChanged: h.calibration_changed(); break;
    case kEvPoseCamParamsChanged: h.pose_cam_params_changed(); break;
    case kEvFinalizeBegins: h.finalize_begins(); break;
    case kEvStructureRebuilt: h.structure_rebuilt(); break;
    case kEvFinalizeSucceeded: h.finalize_succeeded(); break;
    case kEvShardingChanged: h.sharding_changed(); break;
    case kEvPatternBuilt: h.pattern_built(); break;
    case kEvSolveBegins: h.solve_begins(); break;
    case kEvMasksChanged: h.masks_changed(); break;
    case kEvLinearizeBegins: h.linearize_begins(); break;
    case kEvLinearizeWritesA: h.linearize_writes_A(); break;
    case kEvLinearizeSucceeded: h.linearize_succeeded(); break;
    case kEvGnSolveBegins: h.gn_solve_begins(); break;
    case kEvSolvedByPcg: h.solved_by_pcg(); break;
    case kEvSolvedDirectly: h.solved_directly(); break;
    case kEvStandaloneFactorisation: h.standalone_factorisation(); break;
    case kEvPcgRunBegins: h.pcg_run_begins(); break;
    case kEvPcgRunFinishedPlain: h.pcg_run_finished(false); break;
    case kEvPcgRunFinishedCoarse: h.pcg_run_finished(true); break;
    case kEvDoglegSumsOk: h.dogleg_sums(true); break;
    case kEvDoglegSumsFailed: h.dogleg_sums(false); break;
    case kEvStepAppliedTo0: h.step_applied(0); break;
    case kEvStepAppliedTo1: h.step_applied(1); break;
    case kEvRolledBack: h.rolled_back(); break;
    case kEvResidualsEvaluatedAt0: h.residuals_evaluated(0); break;
    case kEvResidualsEvaluatedAt1: h.residuals_evaluated(1); break;
    case kEvSelinvComputed: h.selinv_computed(); break;
    case kEvSelinvReleased: h.selinv_released(); break;
    case kEvMarginalizeFailed: h.marginalize_failed(); break;
    case kEvMarginalized: h.marginalized(); break;
    case kEvMarginalizationReleased: h.marginalization_released(); break;
    case kEvSquareCleared: h.square_cleared(&h); break;   // any non-null address
    case kEvSquareDirty: h.square_dirty(); break;
    default: return false;
  }
  return true;
}

}  // namespace bae
