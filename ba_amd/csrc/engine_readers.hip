// The readers behind include/ba_hip.h: marginals, leverages, joint covariances, factor solves, weakest modes, panel
// PCG, the downloads, statistics and solver switches between them, and the stand-alone solves and test taps.  What a
// request may read and which rows it names is decided in requests.h; the work is in the k_*.hip behind engine.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "entry.h"
#include "factorsolve.h"

namespace bae {

static_assert(kRequestMaxBlock == kPcgMaxBlock, "block_ok of requests.h states the limit of pcg.h");

// The host work that ba_hip_dense_solve, ba_hip_pcg_solve and ba_hip_tile_solve share.  pad_system: the caller's
// n x n lower triangle in (ld + 1) x ld storage, ones on the padded diagonal, the right-hand side as row ld; with
// want_nz also the nt x nt map of the tiles that hold a nonzero entry.
struct PaddedSystem {
  uint32_t ld = 0, nt = 0;
  std::vector<double> A;
  std::vector<uint8_t> nz;
};
static PaddedSystem pad_system(uint32_t n, const double* a_lower, const double* b, bool want_nz) {
  PaddedSystem s;
  const uint32_t ld = s.ld = std::max(((n + 63) / 64) * 64, 64u), nt = s.nt = ld / 64;
  s.A.assign((size_t)(ld + 1) * ld, 0.0);
  if (want_nz) s.nz.assign((size_t)nt * nt, 0);
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = 0; c <= r; ++c) {
      const double v = a_lower[(size_t)r * n + c];
      s.A[(size_t)r * ld + c] = v;
      if (want_nz && v != 0.0) s.nz[(size_t)(r / 64) * nt + c / 64] = 1;
    }
  for (uint32_t r = n; r < ld; ++r) s.A[(size_t)r * ld + r] = 1.0;
  for (uint32_t c = 0; c < n; ++c) s.A[(size_t)ld * ld + c] = b[c];
  return s;
}
// ... and the first n entries of the solution back
static hipError_t download_x(const DBuf<double>& dx, uint32_t n, double* x) {
  return hipMemcpy(x, dx.p, (size_t)n * 8, hipMemcpyDeviceToHost);
}
// `*out = field` of a statistics getter, refused with the function's name when out is NULL
template <typename T>
static int put_stats(Engine* e, const char* who, T* out, const T& v) {
  if (!out) return e->fail_msg((std::string(who) + ": NULL argument").c_str());
  *out = v;
  return 0;
}

}  // namespace bae

using namespace bae;

extern "C" {

// ---- marginal covariances (k_selinv.hip) ----------------------------------------------------------
static int marginals_ready(Engine* e, const char* what, bool landmarks) {
  BA_ASK(guard_marginals(e->held, guard_facts(e), what, landmarks));
  return marginals_compute(e);
}
int ba_hip_compute_marginals(ba_hip_engine* h) {
  BA_ENTRY_DEVICE(h);
  return marginals_ready(e, "ba_hip_compute_marginals", false);
}
int ba_hip_get_pose_marginals(ba_hip_engine* h, uint32_t n, const uint32_t* pose_ids, double* out) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_get_pose_marginals";
  if (int rc = marginals_ready(e, what, false)) return rc;
  if (n && (!pose_ids || !out)) return e->fail_msg("ba_hip_get_pose_marginals: NULL argument");
  const StructureView sv = structure_view(e);
  std::vector<uint32_t> r(n);
  for (uint32_t i = 0; i < n; ++i) BA_ASK(pose_row(sv, what, pose_ids[i], &r[i]));
  return marginals_gather(e, n, r, r, e->pose_dim, e->pose_dim, out);
}
int ba_hip_get_pose_pair_marginals(ba_hip_engine* h, uint32_t n, const uint32_t* a_ids, const uint32_t* b_ids, double* out) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_get_pose_pair_marginals";
  if (int rc = marginals_ready(e, what, false)) return rc;
  if (n && (!a_ids || !b_ids || !out)) return e->fail_msg("ba_hip_get_pose_pair_marginals: NULL argument");
  const StructureView sv = structure_view(e);
  std::vector<uint32_t> ra(n), rb(n);
  for (uint32_t i = 0; i < n; ++i) {
    BA_ASK(pose_row(sv, what, a_ids[i], &ra[i]));
    BA_ASK(pose_row(sv, what, b_ids[i], &rb[i]));
  }
  return marginals_gather(e, n, ra, rb, e->pose_dim, e->pose_dim, out);
}
int ba_hip_get_calibration_block_marginals(ba_hip_engine* h, double* out) {
  BA_ENTRY_DEVICE(h);
  if (!e->st.K) return e->fail_msg("no calibration columns (ba_hip_set_calibration)");
  if (int rc = marginals_ready(e, "ba_hip_get_calibration_block_marginals", false)) return rc;
  std::vector<uint32_t> r(1, e->st.np);
  return marginals_gather(e, 1, r, r, (int)e->st.K, (int)e->st.K, out);
}
int ba_hip_get_landmark_marginals(ba_hip_engine* h, uint32_t n, const uint32_t* lm_ids, double* out) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_get_landmark_marginals";
  if (int rc = marginals_ready(e, what, true)) return rc;
  if (n && !out) return e->fail_msg("ba_hip_get_landmark_marginals: NULL argument");
  BA_ASK(ids_or_all(what, lm_ids, n, e->st.Lact, "the active landmark count"));
  const StructureView sv = structure_view(e);
  for (uint32_t i = 0; lm_ids && i < n; ++i) BA_ASK(landmark_active(sv, what, lm_ids[i]));
  return marginals_landmarks(e, n, lm_ids, out);
}
// ---- leverages of projection residuals (k_lever.hip) ----
int ba_hip_get_projection_leverages(ba_hip_engine* h, uint32_t n, const uint32_t* residual_ids, double* out) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_get_projection_leverages";
  const std::string m = std::string(what) + ": ";
  if (e->lm_dim == 0) return e->fail_msg((m + "LmSize 0 has no projection residuals").c_str());
  if (int rc = marginals_ready(e, what, true)) return rc;
  if (n && !out) return e->fail_msg((m + "NULL argument").c_str());
  BA_ASK(ids_or_all(what, residual_ids, n, e->st.O, "the projection residual count"));
  for (uint32_t i = 0; residual_ids && i < n; ++i) BA_ASK(residual_id_ok(what, residual_ids[i], e->st.O, "a projection"));
  return leverages_run(e, n, residual_ids, out);
}
int ba_hip_get_leverage_stats(ba_hip_engine* h, ba_hip_leverage_stats* out) {
  BA_ENTRY_HOST(h);
  return put_stats(e, __func__, out, e->lstats);
}
// ---- leverages of unary, binary and inertial residuals (k_pplever.hip) ----
int ba_hip_get_pose_pose_leverages(ba_hip_engine* h, int kind, uint32_t n, const uint32_t* ids, double* cov, double* info,
                                   double* leverage) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_get_pose_pose_leverages";
  const std::string m = std::string(what) + ": ";
  if (kind != BA_HIP_RES_UNARY && kind != BA_HIP_RES_BINARY && kind != BA_HIP_RES_IMU)
    return e->fail_msg((m + "kind " + std::to_string(kind) + " is none of BA_HIP_RES_UNARY, _BINARY, _IMU").c_str());
  if (int rc = marginals_ready(e, what, false)) return rc;
  static const char* names[3] = {"a unary", "a binary", "an inertial"};
  const Problem& pb = e->prob;
  const uint32_t count = kind == BA_HIP_RES_UNARY ? pb.num_unary : kind == BA_HIP_RES_BINARY ? pb.num_binary : pb.num_imu;
  if (n && !cov && !info && !leverage) return e->fail_msg((m + "every output is NULL").c_str());
  BA_ASK(ids_or_all(what, ids, n, count, "the residual count of the kind (" + std::to_string(count) + ")"));
  for (uint32_t i = 0; ids && i < n; ++i) BA_ASK(residual_id_ok(what, ids[i], count, names[kind]));
  return pose_pose_leverages_run(e, kind, n, ids, cov, info, leverage);
}
uint32_t ba_hip_num_pose_pose_residuals(const ba_hip_engine* h, int kind) {
  const Problem& pb = reinterpret_cast<const Engine*>(h)->prob;
  return kind == BA_HIP_RES_UNARY ? pb.num_unary : kind == BA_HIP_RES_BINARY ? pb.num_binary : kind == BA_HIP_RES_IMU ? pb.num_imu : 0;
}
int ba_hip_get_pose_pose_leverage_stats(ba_hip_engine* h, ba_hip_pose_pose_leverage_stats* out) {
  BA_ENTRY_HOST(h);
  return put_stats(e, __func__, out, e->ppl_stats);
}
// ---- joint covariance of a pose set (k_jointcov.hip): Y = L^-1 E over the reach, Sigma = Y^T D Y; with landmarks
// the columns [E | -W V^-1] and V^-1 on their diagonal blocks.  One path for both getters: `what` starts the messages.
static int joint_state_run(Engine* e, const char* what, bool state, uint32_t n, const uint32_t* pose_ids,
                           int include_calibration, uint32_t nl, const uint32_t* lm_ids, double* out) {
  if (nl && !e->lm_dim) return e->fail_msg((std::string(what) + ": LmSize 0 has no landmark unknowns").c_str());
  BA_ASK(guard_kept_factor(e->held, guard_facts(e), what, "joint marginals", false, nl != 0));
  RowSelection sel;
  BA_ASK(select_rows(structure_view(e),
                     {what, n, pose_ids, include_calibration != 0, nl, lm_ids, out != nullptr, BA_HIP_JOINT_MAX_COLUMNS,
                      "BA_HIP_JOINT_MAX_COLUMNS",
                      state ? "no pose, no calibration rows and no landmark requested" : "no pose and no calibration rows requested",
                      false},
                     &sel));
  if (int rc = jointcov_run(e, sel.rows, sel.lms, out)) return rc;
  if (state && !nl) e->jsstats = ba_hip_joint_state_stats{};
  return 0;
}
int ba_hip_get_joint_marginals(ba_hip_engine* h, uint32_t n, const uint32_t* pose_ids, int include_calibration,
                               double* out) {
  BA_ENTRY_DEVICE(h);
  return joint_state_run(e, "ba_hip_get_joint_marginals", false, n, pose_ids, include_calibration, 0, nullptr, out);
}
int ba_hip_get_joint_state_marginals(ba_hip_engine* h, uint32_t n_poses, const uint32_t* pose_ids, int include_calibration,
                                     uint32_t n_landmarks, const uint32_t* lm_ids, double* out) {
  BA_ENTRY_DEVICE(h);
  return joint_state_run(e, "ba_hip_get_joint_state_marginals", true, n_poses, pose_ids, include_calibration, n_landmarks,
                         lm_ids, out);
}
int ba_hip_get_joint_state_stats(ba_hip_engine* h, ba_hip_joint_state_stats* out) {
  BA_ENTRY_HOST(h);
  return put_stats(e, __func__, out, e->jsstats);
}
int ba_hip_get_joint_marginal_stats(ba_hip_engine* h, ba_hip_joint_marginal_stats* out) {
  BA_ENTRY_HOST(h);
  return put_stats(e, __func__, out, e->jstats);
}
// ---- solves with the kept factor (k_factorsolve.hip): X = S^-1 B, rows in the caller's (natural) order ----
int ba_hip_factor_solve(ba_hip_engine* h, uint32_t m, const double* B, double* X) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_factor_solve";
  BA_ASK(guard_kept_factor(e->held, guard_facts(e), what, "solves with the factor", false));
  BA_ASK(columns_ok(what, m, BA_HIP_FACTOR_SOLVE_MAX_COLUMNS, "BA_HIP_FACTOR_SOLVE_MAX_COLUMNS"));
  if (!B || !X) return e->fail_msg("ba_hip_factor_solve: NULL argument");
  FactorRef f = {e->A.p, e->st.ld, 0, &e->nzL_host, nullptr, nullptr};
  if (int rc = kept_factor(e, "factor solve", &f.nt, &f.dsgn, &f.linvT)) return rc;
  return factor_solve_run(e, f, e->st.n, natural_rowmap(structure_view(e)).data(), m, B, X);
}
int ba_hip_get_weakest_modes(ba_hip_engine* h, uint32_t k, const ba_hip_mode_options* o, double* eigenvalues,
                             double* modes) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_get_weakest_modes";
  const std::string w = std::string(what) + ": ";
  BA_ASK(guard_kept_factor(e->held, guard_facts(e), what, "weakest modes", false));
  const uint32_t n = e->st.n, kmax = std::min(kModeMaxK, n);
  if (k == 0 || k > kmax)
    return e->fail_msg((w + std::to_string(k) + " modes requested, k must be between 1 and min(32, n) = " +
                        std::to_string(kmax)).c_str());
  if (!eigenvalues || !modes) return e->fail_msg((w + "NULL argument").c_str());
  ModeOptions mo;
  if (o && o->tolerance > 0.0) mo.tolerance = o->tolerance;
  if (o && o->max_iterations) mo.max_iterations = o->max_iterations;
  if (o && o->seed) mo.seed = o->seed;
  FactorRef f = {e->A.p, e->st.ld, 0, &e->nzL_host, nullptr, nullptr};
  if (int rc = kept_factor(e, "weakest modes", &f.nt, &f.dsgn, &f.linvT)) return rc;
  return weakest_modes_run(e, f, n, natural_rowmap(structure_view(e)).data(), k, mo, eigenvalues, modes);
}
int ba_hip_get_mode_stats(ba_hip_engine* h, ba_hip_mode_stats* out) {
  BA_ENTRY_HOST(h);
  return put_stats(e, __func__, out, e->mode_stats);
}
int ba_hip_get_factor_solve_stats(ba_hip_engine* h, ba_hip_factor_solve_stats* out) {
  BA_ENTRY_HOST(h);
  return put_stats(e, __func__, out, e->fsstats);
}
int ba_hip_get_marginal_stats(ba_hip_engine* h, ba_hip_marginal_stats* out) {
  BA_ENTRY_HOST(h);
  return put_stats(e, __func__, out, e->mstats);
}
int ba_hip_release_marginals(ba_hip_engine* h) {
  BA_ENTRY_DEVICE(h);
  (void)hipStreamSynchronize(e->stream);
  marginals_release(e);
  jointcov_release(e);
  factor_solve_release(e);
  e->tri.release();
  e->resect.release();
  return 0;
}

int ba_hip_get_rhs(ba_hip_engine* h, double* rhs_p_sc, double* rhs_p, double* rhs_l) {
  BA_ENTRY_FINAL(h);
  const Structure& st = e->st;
  BAE_HIP(hipStreamSynchronize(e->stream));
  if (rhs_p_sc && st.n) BAE_HIP(hipMemcpy(rhs_p_sc, e->rhs_sc.p, (size_t)st.n * 8, hipMemcpyDeviceToHost));
  if (rhs_p && st.n) BAE_HIP(hipMemcpy(rhs_p, e->rhs_p.p, (size_t)st.n * 8, hipMemcpyDeviceToHost));
  unpermute_vec(e, st.n ? rhs_p_sc : nullptr);
  unpermute_vec(e, st.n ? rhs_p : nullptr);
  if (rhs_l && st.Lact) {
    std::vector<double> bl((size_t)st.L * e->lm_dim);
    BAE_HIP(hipMemcpy(bl.data(), e->lm_bl.p, bl.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t l = 0; l < st.L; ++l)
      if (st.lm_opt[l] >= 0)
        for (int k = 0; k < e->lm_dim; ++k)
          rhs_l[(size_t)st.lm_opt[l] * e->lm_dim + k] = bl[(size_t)l * e->lm_dim + k];
  }
  return 0;
}

// a pose / landmark pair of update vectors to the host, the pose rows in the caller's order
static int download_delta(Engine* e, const DBuf<double>& p, const DBuf<double>& l, double* delta_p, double* delta_l) {
  const Structure& st = e->st;
  BAE_HIP(hipStreamSynchronize(e->stream));
  if (delta_p && st.n) BAE_HIP(hipMemcpy(delta_p, p.p, (size_t)st.n * 8, hipMemcpyDeviceToHost));
  unpermute_vec(e, st.n ? delta_p : nullptr);
  if (delta_l && st.Lact) BAE_HIP(hipMemcpy(delta_l, l.p, (size_t)st.Lact * e->lm_dim * 8, hipMemcpyDeviceToHost));
  return 0;
}
int ba_hip_get_delta_gn(ba_hip_engine* h, double* delta_p, double* delta_l) {
  BA_ENTRY_FINAL(h);
  return download_delta(e, e->gn_p, e->gn_l, delta_p, delta_l);
}
int ba_hip_get_step(ba_hip_engine* h, double* delta_p, double* delta_l) {
  BA_ENTRY_FINAL(h);
  return download_delta(e, e->step_p, e->step_l, delta_p, delta_l);
}

int ba_hip_get_proj_weights(ba_hip_engine* h, double* weight) {
  BA_ENTRY_FINAL(h);
  const Structure& st = e->st;
  std::vector<double> w(st.O);
  BAE_HIP(hipStreamSynchronize(e->stream));
  if (st.O) BAE_HIP(hipMemcpy(w.data(), e->obs_w.p, (size_t)st.O * 8, hipMemcpyDeviceToHost));
  for (uint32_t s = 0; s < st.O; ++s) weight[st.obs_perm[s]] = w[s];
  return 0;
}

int ba_hip_get_proj_residuals(ba_hip_engine* h, double* residual2) {
  BA_ENTRY_FINAL(h);
  const Structure& st = e->st;
  if (st.O == 0) return 0;
  DBuf<double> d;
  BAE_HIP(d.alloc((size_t)2 * st.O));
  int rc = launch_residual_vectors(e, d.p);
  if (rc) return rc;
  std::vector<double> r((size_t)2 * st.O);
  BAE_HIP(hipStreamSynchronize(e->stream));
  BAE_HIP(hipMemcpy(r.data(), d.p, r.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (uint32_t s = 0; s < st.O; ++s) {
    residual2[2 * (size_t)st.obs_perm[s]] = r[2 * (size_t)s];
    residual2[2 * (size_t)st.obs_perm[s] + 1] = r[2 * (size_t)s + 1];
  }
  return 0;
}

int ba_hip_get_proj_jacobians(ba_hip_engine* h, double* j_meas12, double* j_ref12, double* j_lm, double* r2) {
  BA_ENTRY_FINAL(h);
  const Structure& st = e->st;
  if (st.O == 0) return 0;
  BAE_HIP(hipStreamSynchronize(e->stream));
  const int LM = e->lm_dim, R = rows_per_obs(LM);
  std::vector<double> rows((size_t)st.O * R * kRow), jl((size_t)st.O * 2 * LM), sc((size_t)2 * st.O);
  BAE_HIP(hipMemcpy(rows.data(), e->frow.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
  BAE_HIP(hipMemcpy(jl.data(), e->obs_jl.p, jl.size() * sizeof(double), hipMemcpyDeviceToHost));
  BAE_HIP(hipMemcpy(sc.data(), e->scal.p, sc.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (uint32_t s = 0; s < st.O; ++s) {
    const size_t a = st.obs_perm[s];
    const double* rr = &rows[(size_t)s * R * kRow];
    if (j_meas12) for (int i = 0; i < 12; ++i) j_meas12[12 * a + i] = rr[i];
    if (j_ref12) for (int i = 0; i < 12; ++i) j_ref12[12 * a + i] = LM == 1 ? rr[12 + i] : 0.0;
    if (j_lm) for (int i = 0; i < 2 * LM; ++i) j_lm[2 * LM * a + i] = jl[(size_t)s * 2 * LM + i];
    if (r2) { r2[2 * a] = sc[2 * (size_t)s]; r2[2 * a + 1] = sc[2 * (size_t)s + 1]; }
  }
  return 0;
}

// 6 doubles per row: with CalibSize 4 / 5 the last two / the last column are zero
int ba_hip_get_calib_jacobians(ba_hip_engine* h, double* j_k12) {
  BA_ENTRY_FINAL(h);
  const Structure& st = e->st;
  if (!st.K) return e->fail_msg("no calibration columns (ba_hip_set_calibration)");
  if (st.O == 0) return 0;
  BAE_HIP(hipStreamSynchronize(e->stream));
  std::vector<double> rows((size_t)2 * st.O * kRow);
  BAE_HIP(hipMemcpy(rows.data(), e->crow.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (uint32_t s = 0; s < st.O; ++s)
    for (int i = 0; i < 12; ++i) j_k12[12 * (size_t)st.obs_perm[s] + i] = rows[12 * (size_t)s + i];
  return 0;
}

int ba_hip_get_imu_residuals(ba_hip_engine* h, double* residual15) {
  BA_ENTRY_FINAL(h);
  const uint32_t ni = e->prob.num_imu;
  if (ni == 0) return 0;
  DBuf<double> d;
  BAE_HIP(d.alloc((size_t)15 * ni));
  int rc = launch_imu_residual_vectors(e, d.p);
  if (rc) return rc;
  BAE_HIP(hipStreamSynchronize(e->stream));
  BAE_HIP(hipMemcpy(residual15, d.p, (size_t)15 * ni * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int ba_hip_get_imu_errors(ba_hip_engine* h, double* mahalanobis) {
  BA_ENTRY_FINAL(h);
  const Problem& pb = e->prob;
  if (pb.num_imu == 0) return 0;
  BAE_HIP(hipStreamSynchronize(e->stream));
  BAE_HIP(hipMemcpy(mahalanobis, e->pp_err.p + pb.num_unary + pb.num_binary, (size_t)pb.num_imu * sizeof(double),
                    hipMemcpyDeviceToHost));
  return 0;
}

int ba_hip_set_unary_scales(ba_hip_engine* h, uint32_t n, const double* scale) {
  BA_ENTRY_FINAL(h);
  if (n != e->prob.num_unary || (n && !scale)) return e->fail_msg("ba_hip_set_unary_scales: one scale per unary residual expected");
  if (!n) return 0;
  BAE_HIP(hipMemcpyAsync(e->un_scale.p, scale, n * sizeof(double), hipMemcpyHostToDevice, e->stream));
  BAE_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

int ba_hip_get_unary_scales(ba_hip_engine* h, double* scale) {
  BA_ENTRY_FINAL(h);
  BAE_HIP(hipStreamSynchronize(e->stream));
  if (e->prob.num_unary)
    BAE_HIP(hipMemcpy(scale, e->un_scale.p, (size_t)e->prob.num_unary * 8, hipMemcpyDeviceToHost));
  return 0;
}

int ba_hip_check_solve(ba_hip_engine* h, double* residual_norm, double* rhs_norm) {
  BA_ENTRY_FINAL(h);
  BA_ASK(guard_check_solve(e->held, guard_facts(e)));
  double o[2];
  int rc = check_solve_residual(e, e->held.pcg_solved ? e->A.p : e->A_keep.p, e->gn_p.p, e->rhs_sc.p, o);
  if (rc) return rc;
  if (residual_norm) *residual_norm = o[0];
  if (rhs_norm) *rhs_norm = o[1];
  return 0;
}

int ba_hip_get_timers(ba_hip_engine* h, ba_hip_timers* t) {
  BA_ENTRY_HOST(h);
  *t = e->timers;
  return 0;
}

int ba_hip_get_structure_stats(ba_hip_engine* h, ba_hip_structure_stats* out) {
  BA_ENTRY_FINAL(h);
  const Structure& st = e->st;
  memset(out, 0, sizeof(*out));
  out->poses_active = st.Pact; out->landmarks_active = st.Lact; out->observations = st.O;
  out->incidences = st.n_inc; out->factor_rows = st.n_rows;
  out->pair_blocks = st.n_pairs; out->pair_entries = st.n_pair_entries;
  out->tile_refs = st.n_tile_refs; out->pose_entries = st.n_pose_entries; out->linearize_waves = st.n_chunks;
  const uint64_t nt = st.ld / 64;
  out->tiles_lower = nt * (nt + 1) / 2;
  if (!e->held.nzL_valid && !(e->sharded())) {
    int rc = factor_tile_pattern(e);
    if (rc) return rc;
  }
  if (e->held.nzL_valid && e->nzL_host.size() == nt * nt && e->nzS_host.size() == nt * nt)
    for (uint64_t i = 0; i < nt; ++i)
      for (uint64_t k = 0; k <= i; ++k) {
        out->tiles_S += e->nzS_host[i * nt + k] ? 1 : 0;
        out->tiles_L += e->nzL_host[i * nt + k] ? 1 : 0;
      }
  if (e->held.nzL_valid && e->nzL_host.size() == nt * nt) out->factor_tile_products = factor_tile_products(e->nzL_host, (uint32_t)nt);
  return 0;
}

int ba_hip_debug_set(ba_hip_engine* h, int key, int value) {
  BA_ENTRY_HOST(h);
  switch (key) {
    case 1:
      if (value != 0 && value != 1 && value != 2 && value != 5 && value != 6)
        return e->fail_msg("ba_hip_debug_set: key 1 takes the assembly variants 0, 1, 2, 5 and 6");
      e->dbg_assemble_variant = value;
      break;
    case 2: e->dbg_tile_order = value; e->tile_order_version = ~0ull; break;
    case 4: e->dbg_linearize_variant = value; break;
    case 5: e->dbg_host_structure = value; e->held.problem_changed(); break;
    case 6: e->dbg_imu_wave = value; break;
    case 3: e->dbg_all_tiles = value; e->tile_order_version = ~0ull; e->held.square_dirty(); break;
    default: return e->fail_msg("ba_hip_debug_set: unknown key");
  }
  return 0;
}

int ba_hip_set_profiling(ba_hip_engine* h, int enable) {
  BA_ENTRY_DEVICE(h);
  e->prof_collect();
  e->profiling = enable != 0;
  memset(&e->kstats, 0, sizeof(e->kstats));
  return 0;
}
int ba_hip_get_kernel_stats(ba_hip_engine* h, ba_hip_kernel_stats* out) {
  BA_ENTRY_DEVICE(h);
  (void)hipStreamSynchronize(e->stream);
  e->prof_collect();
  *out = e->kstats;
  return 0;
}

int ba_hip_device_buffer(ba_hip_engine* h, int which, void** dev_ptr, size_t* num_doubles) {
  BA_ENTRY_HOST(h);
  if (!e->held.finalized) return e->fail_msg(kNotFinalized);
  if (which == 0) { *dev_ptr = e->A.p; *num_doubles = (size_t)(e->st.ld + 1) * e->st.ld; return 0; }
  if (which == 1) { *dev_ptr = e->scalars_out.p; *num_doubles = e->scalars_out.n; return 0; }
  return e->fail_msg("unknown buffer id");
}

int ba_hip_allreduce_host(ba_hip_engine* h, void* host, size_t count, int dtype) {
  BA_ENTRY_DEVICE(h);
  if (!e->sharded() || count == 0) return 0;  // single shard: the values are already the totals
  DBuf<double> d;  // both element types are 8 bytes
  BAE_HIP(d.alloc(count));
  hipError_t err = hipMemcpy(d.p, host, count * 8, hipMemcpyHostToDevice);
  int rc = 0;
  if (err != hipSuccess) rc = e->fail(err, "hipMemcpy");
  if (!rc && shard_allreduce(e, d.p, count, dtype) != 0) rc = e->fail_msg("allreduce hook failed");
  if (!rc && (err = hipMemcpy(host, d.p, count * 8, hipMemcpyDeviceToHost)) != hipSuccess) rc = e->fail(err, "hipMemcpy");
  return rc;
}

int ba_hip_get_comm_stats(ba_hip_engine* h, ba_hip_comm_stats* out) {
  BA_ENTRY_HOST(h);
  if (!out) return e->fail_msg("null output");
  *out = e->cstats;
  return 0;
}

int ba_hip_reset_comm_stats(ba_hip_engine* h) {
  BA_ENTRY_HOST(h);
  memset(&e->cstats, 0, sizeof(e->cstats));
  return 0;
}

int ba_hip_dist_plan_stats(uint32_t nblk, const uint8_t* nz_lower, int nranks, const char* layout, uint32_t kout,
                           ba_hip_dist_plan_stats_t* out) {
  if (!out || nranks < 1 || nblk == 0) return -1;
  const uint32_t G = kout ? kout : choose_kout(nblk);
  OwnMap map;
  std::string name;
  if (!build_own_map((uint32_t)nranks, layout, G, &map, &name)) return -1;
  const DistPlanStats s = dist_plan_stats(build_dist_plan(nblk, map, nz_lower));
  out->factor_bytes = s.factor_bytes;
  out->chain_recv_max = s.chain_recv_max; out->chain_recv_total = s.chain_recv_total;
  out->side_recv_max = s.side_recv_max; out->side_recv_total = s.side_recv_total;
  out->chain_sent_total = s.chain_sent_total; out->side_sent_total = s.side_sent_total;
  out->recv_max = s.recv_max; out->backward_allreduce_bytes = s.backward_allreduce_bytes;
  out->messages_chain = s.messages_chain; out->messages_side = s.messages_side;
  out->panels = s.panels; out->ranks = s.ranks; out->classes = s.classes; out->kout = G;
  return 0;
}

int ba_hip_get_factor_tile_pattern(ba_hip_engine* h, uint32_t nblk, uint8_t* nz_lower) {
  BA_ENTRY_FINAL(h);
  if (!e->held.nzL_valid) {
    const int rc = factor_tile_pattern(e);
    if (rc) return rc;
  }
  if (e->nzL_host.size() != (size_t)nblk * nblk) return e->fail_msg("tile count mismatch");
  memcpy(nz_lower, e->nzL_host.data(), e->nzL_host.size());
  return 0;
}

int ba_hip_solve_is_distributed(ba_hip_engine* h) {
  if (!h) return 0;
  return dist_solve_enabled(reinterpret_cast<Engine*>(h)) ? 1 : 0;
}

int ba_hip_set_pose_ordering(ba_hip_engine* h, int mode) {
  BA_ENTRY_HOST(h);
  if (mode != kOrderNatural && mode != kOrderAuto && mode != kOrderUser)
    return e->fail_msg("ba_hip_set_pose_ordering: unknown mode");
  if (mode != kOrderNatural && e->ordering_refused())
    return e->fail_msg("pose ordering is not available on a sharded engine (all-reduce hook, collectives hook or communicator set)");
  e->order_mode = mode;
  return 0;
}

int ba_hip_set_reduced_solver(ba_hip_engine* h, int mode, const ba_hip_pcg_options* o) {
  BA_ENTRY_HOST(h);
  if (mode != BA_HIP_SOLVER_DIRECT && mode != BA_HIP_SOLVER_PCG) return e->fail_msg("ba_hip_set_reduced_solver: unknown mode");
  if (mode == BA_HIP_SOLVER_PCG) {
    if (e->pcg_refused())
      return e->fail_msg("the PCG solver is not available on a sharded engine (all-reduce hook, collectives hook or communicator set)");
    ba_hip_pcg_options v = {};
    v.rel_tolerance = 1e-6;
    if (o) v = *o;
    BA_ASK(pcg_options_ok("ba_hip_set_reduced_solver", {v.rel_tolerance, v.coarse_aggregate}, kCoarseAllowed));
    e->pcg_opt = v;
  }
  e->solver_mode = mode;
  return 0;
}

int ba_hip_get_pcg_stats(ba_hip_engine* h, ba_hip_pcg_stats* out) {
  BA_ENTRY_HOST(h);
  BA_ASK(guard_pcg_stats(e->held));
  if (out) *out = e->pcg_stats;
  return 0;
}

int ba_hip_get_pcg_coarse_stats(ba_hip_engine* h, ba_hip_pcg_coarse_stats* out) {
  BA_ENTRY_HOST(h);
  BA_ASK(guard_pcg_coarse_stats(e->held));
  if (out) *out = e->pcg_coarse_stats;
  return 0;
}

int ba_hip_get_pcg_coarse(ba_hip_engine* h, uint32_t nc, double* C, double* Cinv) {
  BA_ENTRY_DEVICE(h);
  Engine::PcgWork& w = e->pcg;
  if (!e->held.pcg_coarse_last || !w.coarse_nc || !w.C.p || !w.Cinv.p)
    return e->fail_msg("ba_hip_get_pcg_coarse: the last solve did not use the coarse space");
  if (nc != w.coarse_nc) return e->fail_msg("ba_hip_get_pcg_coarse: nc differs from the coarse unknowns of the last solve");
  const double* src[2] = {w.C.p, w.Cinv.p};
  double* dst[2] = {C, Cinv};
  for (int i = 0; i < 2; ++i)
    if (dst[i])
      BAE_HIP(hipMemcpy2D(dst[i], (size_t)nc * sizeof(double), src[i], (size_t)w.coarse_ncp * sizeof(double),
                          (size_t)nc * sizeof(double), nc, hipMemcpyDeviceToHost));
  return 0;
}

// ---- panel PCG (k_pcg_panel.hip): S^-1 on a block of columns after a PCG solve, A holds S ----
// The refusals the two entry points share; `who` starts the messages.
static int pcg_panel_ready(Engine* e, const char* who, const ba_hip_pcg_options* o) {
  const PcgAsk ask = {o ? o->rel_tolerance : 0.0, o ? o->coarse_aggregate : 0u};
  BA_ASK(guard_pcg_panel(e->held, guard_facts(e), who, o ? &ask : nullptr));
  return 0;
}
// rows in the caller's (natural) order, as ba_hip_factor_solve
static int pcg_panel_on_S(Engine* e, uint32_t m, const double* B, double* X, const ba_hip_pcg_options& o) {
  int status = 0;
  int rc = pcg_panel_solve_device(e, e->A.p, e->st.n, e->st.ld, e->pcg_plan, e->nzS_host, e->pcg_blk, e->pcg_blocks,
                                  natural_rowmap(structure_view(e)).data(), m, B, X, o, &status);
  if (rc) return rc;
  return status ? BA_HIP_FACTORIZATION_ERROR : 0;
}
int ba_hip_pcg_panel_solve_system(ba_hip_engine* h, uint32_t m, const double* B, double* X, const ba_hip_pcg_options* o) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_pcg_panel_solve_system";
  if (int rc = pcg_panel_ready(e, what, o)) return rc;
  BA_ASK(columns_ok(what, m, BA_HIP_PCG_PANEL_MAX_COLUMNS, "BA_HIP_PCG_PANEL_MAX_COLUMNS"));
  if (!B || !X) return e->fail_msg("ba_hip_pcg_panel_solve_system: NULL argument");
  return pcg_panel_on_S(e, m, B, X, *o);
}
int ba_hip_get_joint_marginals_pcg(ba_hip_engine* h, uint32_t n, const uint32_t* pose_ids, int include_calibration,
                                   const ba_hip_pcg_options* o, double* out) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_get_joint_marginals_pcg";
  if (int rc = pcg_panel_ready(e, what, o)) return rc;
  RowSelection s;   // the selected rows in the caller's numbering
  BA_ASK(select_rows(structure_view(e),
                     {what, n, pose_ids, include_calibration != 0, 0, nullptr, out != nullptr, BA_HIP_PCG_PANEL_MAX_COLUMNS,
                      "BA_HIP_PCG_PANEL_MAX_COLUMNS", "no columns requested (m == 0)", true},
                     &s));
  const std::vector<uint32_t>& sel = s.rows;
  const uint32_t m = (uint32_t)sel.size(), N = e->st.n;
  std::vector<double> E((size_t)N * m, 0.0), X((size_t)N * m, 0.0);
  for (uint32_t c = 0; c < m; ++c) E[(size_t)sel[c] * m + c] = 1.0;
  const int rc = pcg_panel_on_S(e, m, E.data(), X.data(), *o);
  if (rc && rc != BA_HIP_FACTORIZATION_ERROR) return rc;
  for (uint32_t a = 0; a < m; ++a)
    for (uint32_t c = 0; c < m; ++c)
      out[(size_t)a * m + c] = 0.5 * (X[(size_t)sel[a] * m + c] + X[(size_t)sel[c] * m + a]);
  return rc;
}
int ba_hip_get_pcg_panel_stats(ba_hip_engine* h, ba_hip_pcg_panel_stats* out) {
  BA_ENTRY_HOST(h);
  return put_stats(e, __func__, out, e->pcgp_stats);
}
int ba_hip_get_pcg_panel_columns(ba_hip_engine* h, uint32_t m, uint32_t* iterations, uint32_t* converged, uint32_t* breakdown,
                                 double* rel_residual_true) {
  BA_ENTRY_HOST(h);
  if (e->pcgp_cols.empty()) return e->fail_msg("ba_hip_get_pcg_panel_columns: no panel solve yet");
  if (m != e->pcgp_cols.size())
    return e->fail_msg(("ba_hip_get_pcg_panel_columns: m differs from the " + std::to_string(e->pcgp_cols.size()) +
                        " columns of the last panel solve").c_str());
  for (uint32_t j = 0; j < m; ++j) {
    const PcgState& c = e->pcgp_cols[j];
    if (iterations) iterations[j] = c.iterations;
    if (converged) converged[j] = c.converged;
    if (breakdown) breakdown[j] = c.breakdown;
    if (rel_residual_true) rel_residual_true[j] = c.bb > 0.0 ? sqrt(c.rr_true / c.bb) : 0.0;
  }
  return 0;
}

// ---- landmark triangulation and per-landmark refinement, poses held fixed (k_triang.hip, triang.h) ----
int ba_hip_triangulate_landmarks(ba_hip_engine* h, uint32_t n, const uint32_t* lm_ids, const ba_hip_triangulation_options* o,
                                 double* result8, double* x_w4) {
  BA_ENTRY_FINAL(h);
  BA_ASK(guard_triangulate(e->held, guard_facts(e), e->st.K != 0 || e->calib_dim != 0, e->lm_dim, e->in_solve));
  // (the cameras as ba_hip_begin_solve takes them)
  if (!e->prob.pose_cam_params.empty() && e->prob.pose_cam_params.size() != 4 * (size_t)e->prob.num_poses)
    return e->fail_msg("per-pose camera parameters: one [fx,fy,u0,v0] per pose expected");
  if (!e->prob.pose_cam_params.empty() && e->has_fov)
    return e->fail_msg("per-pose camera parameters are offered for LinearCamera rigs only");
  TriOptions t;   // the defaults of the header
  if (o) {
    t.linear_init = o->linear_init != 0; t.max_iterations = o->max_iterations; t.write_back = o->write_back != 0;
    t.lambda0 = o->lambda0; t.gradient_tolerance = o->gradient_tolerance; t.step_tolerance = o->step_tolerance;
    t.min_parallax = o->min_parallax; t.huber_width = o->huber_width;
  }
  const Structure& st = e->st;
  const uint32_t L = st.L;
  BA_ASK(triangulation_ok({t.max_iterations, t.lambda0, t.gradient_tolerance, t.step_tolerance, t.min_parallax, t.huber_width},
                          L, n, lm_ids));
  Engine::Tri& w = e->tri;
  w.stats = ba_hip_triangulation_stats();
  w.stats.landmarks = n;
  if (L == 0) return 0;
  std::vector<uint8_t> mask(L, lm_ids ? 0 : 1);
  for (uint32_t i = 0; lm_ids && i < n; ++i) mask[lm_ids[i]] = 1;
  BAE_HIP(w.mask.alloc(L));
  BAE_HIP(w.early.alloc(std::max<size_t>(st.n_chunks, 1)));
  BAE_HIP(w.res.alloc((size_t)L * kTriResult));
  BAE_HIP(w.xw.alloc((size_t)L * 4));
  Events<2> ev;
  BAE_HIP(ev.create());
  BAE_HIP(ev.record(0, e->stream));
  BAE_HIP(hipMemcpyAsync(w.mask.p, mask.data(), L, hipMemcpyHostToDevice, e->stream));
  int rc = launch_pose_prep(e);
  if (!rc) rc = launch_triangulate(e, t);
  if (rc) return rc;
  BAE_HIP(ev.record(1, e->stream));
  BAE_HIP(hipStreamSynchronize(e->stream));
  std::vector<double> res((size_t)L * kTriResult), xw((size_t)L * 4);
  std::vector<uint8_t> early(st.n_chunks);
  BAE_HIP(hipMemcpy(res.data(), w.res.p, res.size() * sizeof(double), hipMemcpyDeviceToHost));
  BAE_HIP(hipMemcpy(xw.data(), w.xw.p, xw.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (st.n_chunks && st.O) BAE_HIP(hipMemcpy(early.data(), w.early.p, early.size(), hipMemcpyDeviceToHost));
  w.stats.device_ms = ev.ms(0, 1);
  w.stats.waves = st.O ? st.n_chunks : 0;
  for (uint8_t v : early) w.stats.waves_early += v ? 1 : 0;
  for (uint32_t i = 0; i < n; ++i) {
    const size_t l = lm_ids ? lm_ids[i] : i;
    const double* r = &res[l * kTriResult];
    const int status = (int)r[0];
    if (status >= 0 && status < kTriStatusCount) w.stats.count[status] += 1;
    // (what tri_accepted decided on the device: OK, or NOT_CONVERGED whose cost fell)
    if (status == kTriOk || (status == kTriNotConverged && (t.linear_init ? r[4] <= r[3] : r[4] < r[3]))) w.stats.written += 1;
    if (result8) std::copy(r, r + kTriResult, result8 + (size_t)i * kTriResult);
    if (x_w4) std::copy(&xw[l * 4], &xw[l * 4] + 4, x_w4 + (size_t)i * 4);
  }
  if (!t.write_back) { w.stats.written = 0; return 0; }
  // accepted rows hold the new coordinates, every other row the bits it had
  BAE_HIP(hipMemcpyAsync(e->lm_xw.p, w.xw.p, (size_t)L * 4 * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  if (e->lm_dim == 3)
    BAE_HIP(hipMemcpyAsync(e->lm_x[e->cur].p, w.xw.p, (size_t)L * 4 * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  else if ((rc = launch_begin_solve(e)))   // x_s from the new x_w
    return rc;
  e->held.solve_begins();   // the landmarks moved: the linearisation and the cached errors are those of other coordinates
  BAE_HIP(hipStreamSynchronize(e->stream));
  return 0;
}
int ba_hip_get_triangulation_stats(ba_hip_engine* h, ba_hip_triangulation_stats* out) {
  BA_ENTRY_HOST(h);
  return put_stats(e, __func__, out, e->tri.stats);
}

// ---- pose refinement with the landmarks held fixed (k_resect.hip, resect.h) ----
// the per-pose observation list of the structure the device holds (the host copies of the sorted observations are gone
// after ba_hip_finalize: obs_pose comes back from the device, once per structure)
static int resect_ensure_lists(Engine* e) {
  Engine::Resect& w = e->resect;
  if (w.list_valid) return 0;
  const Structure& st = e->st;
  std::vector<uint32_t> obs_pose(st.O), idx;
  if (st.O) {
    BAE_HIP(hipStreamSynchronize(e->stream));
    BAE_HIP(hipMemcpy(obs_pose.data(), e->obs_pose.p, (size_t)st.O * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  if (!build_pose_obs_lists(st.P, st.O, obs_pose.data(), &w.host_ptr, &idx))
    return e->fail_msg("ba_hip_refine_poses: an observation names a pose that does not exist");
  BAE_HIP(w.ptr.alloc((size_t)st.P + 1));
  BAE_HIP(w.idx.alloc(std::max<size_t>(st.O, 1)));
  BAE_HIP(w.used.alloc(std::max<size_t>(st.O, 1)));
  BAE_HIP(hipMemcpy(w.ptr.p, w.host_ptr.data(), ((size_t)st.P + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (st.O) BAE_HIP(hipMemcpy(w.idx.p, idx.data(), (size_t)st.O * sizeof(uint32_t), hipMemcpyHostToDevice));
  w.list_valid = true;
  return 0;
}

int ba_hip_refine_poses(ba_hip_engine* h, uint32_t n, const uint32_t* pose_ids, const ba_hip_pose_refinement_options* o,
                        double* result8, double* t_wp7, double* info36) {
  BA_ENTRY_FINAL(h);
  BA_ASK(guard_refine_poses(e->held, guard_facts(e), e->st.K != 0 || e->calib_dim != 0, e->lm_dim, e->in_solve));
  // (the cameras as ba_hip_begin_solve takes them)
  if (!e->prob.pose_cam_params.empty() && e->prob.pose_cam_params.size() != 4 * (size_t)e->prob.num_poses)
    return e->fail_msg("per-pose camera parameters: one [fx,fy,u0,v0] per pose expected");
  if (!e->prob.pose_cam_params.empty() && e->has_fov)
    return e->fail_msg("per-pose camera parameters are offered for LinearCamera rigs only");
  RsOptions t;   // the defaults of the header
  if (o) {
    t.max_iterations = o->max_iterations; t.write_back = o->write_back != 0; t.fixed_mask = o->fixed_mask;
    t.lambda0 = o->initial_damping; t.gradient_tolerance = o->gradient_tolerance; t.step_tolerance = o->step_tolerance;
    t.huber_width = o->huber_width;
  }
  const Structure& st = e->st;
  const uint32_t P = st.P;
  BA_ASK(refinement_ok({t.max_iterations, t.fixed_mask, t.lambda0, t.gradient_tolerance, t.step_tolerance, t.huber_width}, P,
                       n, pose_ids));
  Engine::Resect& w = e->resect;
  w.stats = ba_hip_pose_refinement_stats();
  w.stats.poses = n;
  int rc = resect_ensure_lists(e);
  if (rc) return rc;
  // the requests grouped by launch: no observations | up to 256 | up to 1 024 | more; rows: their place in the request
  uint32_t cls[4] = {0, 0, 0, 0};
  auto cls_of = [&](uint32_t p) {
    const uint32_t k = w.host_ptr[p + 1] - w.host_ptr[p];
    return k == 0 ? 0 : k <= 256 ? 1 : k <= 1024 ? 2 : 3;
  };
  for (uint32_t i = 0; i < n; ++i) cls[cls_of(pose_ids ? pose_ids[i] : i)] += 1;
  uint32_t at[4] = {0, cls[0], cls[0] + cls[1], cls[0] + cls[1] + cls[2]};
  // (held by the work space, and kept by its release(): the uploads below are asynchronous, and an error return must
  // not leave them reading freed memory)
  std::vector<uint32_t>& ids = w.host_ids;
  std::vector<uint32_t>& rows = w.host_rows;
  ids.assign(n, 0); rows.assign(n, 0);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t p = pose_ids ? pose_ids[i] : i, j = at[cls_of(p)]++;
    ids[j] = p; rows[j] = i;
  }
  BAE_HIP(w.ids.alloc(n)); BAE_HIP(w.rows.alloc(n));
  BAE_HIP(w.res.alloc((size_t)n * kRsResult)); BAE_HIP(w.t7.alloc((size_t)n * 7)); BAE_HIP(w.info.alloc((size_t)n * 36));
  Events<2> ev;
  BAE_HIP(ev.create());
  BAE_HIP(ev.record(0, e->stream));
  BAE_HIP(hipMemcpyAsync(w.ids.p, ids.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  BAE_HIP(hipMemcpyAsync(w.rows.p, rows.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  rc = launch_pose_prep(e);
  if (!rc) rc = launch_resect(e, t, cls);
  if (rc) return rc;
  BAE_HIP(ev.record(1, e->stream));
  BAE_HIP(hipStreamSynchronize(e->stream));
  std::vector<double> res((size_t)n * kRsResult);
  BAE_HIP(hipMemcpy(res.data(), w.res.p, res.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (t_wp7) BAE_HIP(hipMemcpy(t_wp7, w.t7.p, (size_t)n * 7 * sizeof(double), hipMemcpyDeviceToHost));
  if (info36) BAE_HIP(hipMemcpy(info36, w.info.p, (size_t)n * 36 * sizeof(double), hipMemcpyDeviceToHost));
  w.stats.device_ms = ev.ms(0, 1);
  for (uint32_t i = 0; i < n; ++i) {
    const double* r = &res[(size_t)i * kRsResult];
    const int status = (int)r[0];
    if (status >= 0 && status < kRsStatusCount) w.stats.count[status] += 1;
    if (rs_row_accepted(r)) w.stats.written += 1;   // (what rs_accepted decided on the device)
    w.stats.observations_used += (uint64_t)r[1];
    w.stats.observations_excluded += (uint64_t)r[7];
  }
  if (result8) std::copy(res.begin(), res.end(), result8);
  if (!t.write_back) { w.stats.written = 0; return 0; }
  // accepted rows hold the new pose, every other requested row the bits it had
  if ((rc = launch_resect_store(e, n))) return rc;
  if (e->lm_dim == 1) {   // x_s from the x_w that stayed, in the reference sensors that moved
    if ((rc = launch_pose_prep(e))) return rc;
    if ((rc = launch_begin_solve(e))) return rc;
  }
  e->held.solve_begins();   // the poses moved: the linearisation and the cached errors are those of other poses
  BAE_HIP(hipStreamSynchronize(e->stream));
  return 0;
}
int ba_hip_get_pose_refinement_stats(ba_hip_engine* h, ba_hip_pose_refinement_stats* out) {
  BA_ENTRY_HOST(h);
  return put_stats(e, __func__, out, e->resect.stats);
}

int ba_hip_dense_solve(ba_hip_engine* h, uint32_t n, const double* a_lower, const double* b, double* x) {
  BA_ENTRY_DEVICE(h);
  const PaddedSystem sys = pad_system(n, a_lower, b, false);
  DBuf<double> dA, dx;
  BAE_HIP(dA.alloc(sys.A.size()));
  BAE_HIP(dx.alloc(sys.ld));
  BAE_HIP(e->flags.alloc(16));
  BAE_HIP(hipMemcpy(dA.p, sys.A.data(), sys.A.size() * 8, hipMemcpyHostToDevice));
  int status = 0;
  e->held.standalone_factorisation();
  int rc = cholesky_solve(e, dA.p, n, sys.ld, dx.p, &status, nullptr);  // arbitrary matrix: dense
  if (rc) return rc;
  BAE_HIP(download_x(dx, n, x));
  return status ? BA_HIP_FACTORIZATION_ERROR : 0;
}

int ba_hip_pcg_solve(ba_hip_engine* h, uint32_t n, const double* a_lower, const double* b, uint32_t block,
                     const ba_hip_pcg_options* o, double* x, ba_hip_pcg_stats* stats) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_pcg_solve";
  if (!n || !a_lower || !b || !o || !x) return e->fail_msg("ba_hip_pcg_solve: NULL or empty argument");
  BA_ASK(block_ok(what, block));
  BA_ASK(pcg_options_ok(what, {o->rel_tolerance, o->coarse_aggregate}, kCoarseAllowed));
  const PaddedSystem sys = pad_system(n, a_lower, b, true);
  const uint32_t ld = sys.ld;
  PcgPlan plan;
  build_pcg_plan(sys.nz, sys.nt, plan);
  std::vector<uint32_t> blk, blocks;
  pcg_row_blocks(n, block, 0, ld, blk, blocks);
  if (o->coarse_aggregate) {
    std::vector<uint32_t> nat;
    uint32_t nblk = 0;
    pcg_natural_rows(n, block, 0, ld, nat, nblk);
    build_pcg_coarse(plan, nat, nblk, block, 0, o->coarse_aggregate);
  }
  DBuf<double> dA, dx;
  BAE_HIP(dA.alloc(sys.A.size()));
  BAE_HIP(dx.alloc(ld));
  BAE_HIP(hipMemcpy(dA.p, sys.A.data(), sys.A.size() * 8, hipMemcpyHostToDevice));
  int status = 0;
  ba_hip_pcg_stats st;
  e->pcg_plan_version = ~0ull;   // the work space now holds this system's plan, not the engine's
  int rc = pcg_solve_device(e, dA.p, n, ld, dA.p + (size_t)ld * ld, plan, sys.nz, blk, blocks, true, *o, dx.p, &st, &status);
  if (rc) return rc;
  BAE_HIP(download_x(dx, n, x));
  if (stats) *stats = st;
  return status ? BA_HIP_FACTORIZATION_ERROR : 0;
}

int ba_hip_pcg_panel_solve(ba_hip_engine* h, uint32_t n, const double* a_lower, uint32_t m, const double* B, uint32_t block,
                           const ba_hip_pcg_options* o, double* X, ba_hip_pcg_panel_stats* stats) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_pcg_panel_solve";
  if (!n || !a_lower || !o) return e->fail_msg("ba_hip_pcg_panel_solve: NULL or empty argument");
  BA_ASK(columns_ok(what, m, BA_HIP_PCG_PANEL_MAX_COLUMNS, "BA_HIP_PCG_PANEL_MAX_COLUMNS"));
  if (!B || !X) return e->fail_msg("ba_hip_pcg_panel_solve: NULL argument");
  BA_ASK(block_ok(what, block));
  const PcgAsk ask = {o->rel_tolerance, o->coarse_aggregate};
  BA_ASK(pcg_options_ok(what, ask, kCoarseRefusedLast));
  const std::vector<double> zero(n, 0.0);
  const PaddedSystem sys = pad_system(n, a_lower, zero.data(), true);
  const uint32_t ld = sys.ld;
  PcgPlan plan;
  build_pcg_plan(sys.nz, sys.nt, plan);
  std::vector<uint32_t> blk, blocks;
  pcg_row_blocks(n, block, 0, ld, blk, blocks);
  DBuf<double> dA;
  BAE_HIP(dA.alloc(sys.A.size()));
  BAE_HIP(hipMemcpy(dA.p, sys.A.data(), sys.A.size() * 8, hipMemcpyHostToDevice));
  int status = 0;
  e->held.pcg_run_begins();   // a stand-alone PCG run without the coarse space, as ba_hip_pcg_solve
  const int rc = pcg_panel_solve_device(e, dA.p, n, ld, plan, sys.nz, blk, blocks, identity_rowmap(n, ld).data(), m, B, X, *o, &status);
  if (rc) return rc;
  e->held.pcg_run_finished(false);
  if (stats) *stats = e->pcgp_stats;
  return status ? BA_HIP_FACTORIZATION_ERROR : 0;
}

// The direct tile-sparse factorisation on a host system with a caller-supplied tile pattern (test entry: the
// kept factor comes back as the engine holds it).  Uses buffers of its own for the matrix and the pattern; the
// engine's invdiag work space is shared with ba_hip_solve_gn, so the scene's kept factor is marked gone.
// Shared by ba_hip_tile_solve and ba_hip_tile_factor_solve: `who` starts the messages; sys, dA and dx are the
// caller's and outlive the call (the factor stays in dA, its closed pattern in sys.nz, the solution in dx).
static int tile_factorise(Engine* e, const char* who, uint32_t n, const double* a_lower, const double* b,
                          const uint8_t* tile_map, PaddedSystem& sys, DBuf<double>& dA, DBuf<double>& dx, int* status) {
  sys = pad_system(n, a_lower, b, true);
  const uint32_t ld = sys.ld, nt = sys.nt;
  std::vector<uint8_t>& nz = sys.nz;
  if (tile_map) {
    for (uint32_t r = 0; r < n; ++r)
      for (uint32_t c = 0; c <= r; ++c)
        if (a_lower[(size_t)r * n + c] != 0.0 && r / 64 != c / 64 && !tile_map[(size_t)(r / 64) * nt + c / 64]) {
          e->err = std::string(who) + ": entry (" + std::to_string(r) + ", " + std::to_string(c) + ") is nonzero but tile (" +
                   std::to_string(r / 64) + ", " + std::to_string(c / 64) + ") is not in the tile map";
          return -1;
        }
    for (uint32_t i = 0; i < nt; ++i)
      for (uint32_t k = 0; k <= i; ++k) nz[(size_t)i * nt + k] |= tile_map[(size_t)i * nt + k] ? 1 : 0;
  }
  for (uint32_t i = 0; i < nt; ++i) nz[(size_t)i * nt + i] = 1;  // diagonal tiles always
  tile_symbolic_factor(nz, nt);
  DBuf<uint8_t> dnz;
  BAE_HIP(dA.alloc(sys.A.size()));
  BAE_HIP(dx.alloc(ld));
  BAE_HIP(dnz.alloc(nz.size()));
  BAE_HIP(e->flags.alloc(16));
  BAE_HIP(hipMemcpy(dA.p, sys.A.data(), sys.A.size() * 8, hipMemcpyHostToDevice));
  BAE_HIP(hipMemcpy(dnz.p, nz.data(), nz.size(), hipMemcpyHostToDevice));
  e->held.standalone_factorisation();
  BulkDeviceLists lists;            // of this pattern alone: temporary, as dnz
  int rc = ensure_bulk_lists(e, nt, nz.data(), ~0ull, &lists);
  if (rc) return rc;
  rc = cholesky_solve(e, dA.p, n, ld, dx.p, status, dnz.p, &lists);
  if (rc) return rc;
  BAE_HIP(hipDeviceSynchronize());  // both streams of the factorisation (dnz and lists go with this scope)
  return 0;
}
int ba_hip_tile_solve(ba_hip_engine* h, uint32_t n, const double* a_lower, const double* b, const uint8_t* tile_map,
                      double* x, uint8_t* nz_factor, double* factor, double* linvT, double* dsgn) {
  BA_ENTRY_DEVICE(h);
  if (!n || !a_lower || !b || !x) return e->fail_msg("ba_hip_tile_solve: NULL or empty argument");
  PaddedSystem sys;
  DBuf<double> dA, dx;
  int status = 0;
  if (int rc = tile_factorise(e, "ba_hip_tile_solve", n, a_lower, b, tile_map, sys, dA, dx, &status)) return rc;
  const uint32_t ld = sys.ld, nt = sys.nt;
  if (nz_factor) std::copy(sys.nz.begin(), sys.nz.end(), nz_factor);
  hipError_t err = download_x(dx, n, x);
  if (err == hipSuccess && factor) err = hipMemcpy(factor, dA.p, (size_t)ld * ld * 8, hipMemcpyDeviceToHost);
  const FactorWork fw(nt);
  if (err == hipSuccess && dsgn) err = hipMemcpy(dsgn, e->invdiag.p + fw.dsgn, (size_t)ld * 8, hipMemcpyDeviceToHost);
  if (err == hipSuccess && linvT)
    err = hipMemcpy(linvT, e->invdiag.p + fw.linvT, (size_t)nt * 64 * 64 * 8, hipMemcpyDeviceToHost);
  if (err != hipSuccess) return e->fail(err, "hipMemcpy");
  return status ? BA_HIP_FACTORIZATION_ERROR : 0;
}

int ba_hip_tile_factor_solve(ba_hip_engine* h, uint32_t n, const double* a_lower, const uint8_t* tile_map, uint32_t m,
                             const double* B, double* X) {
  BA_ENTRY_DEVICE(h);
  static const char* what = "ba_hip_tile_factor_solve";
  if (!n || !a_lower) return e->fail_msg("ba_hip_tile_factor_solve: NULL or empty argument");
  BA_ASK(columns_ok(what, m, BA_HIP_FACTOR_SOLVE_MAX_COLUMNS, "BA_HIP_FACTOR_SOLVE_MAX_COLUMNS"));
  if (!B || !X) return e->fail_msg("ba_hip_tile_factor_solve: NULL argument");
  PaddedSystem sys;
  DBuf<double> dA, dx;
  int status = 0;
  const std::vector<double> b(n, 0.0);
  if (int rc = tile_factorise(e, what, n, a_lower, b.data(), tile_map, sys, dA, dx, &status)) return rc;
  if (status) return BA_HIP_FACTORIZATION_ERROR;
  const FactorWork fw(sys.nt);
  const FactorRef f = {dA.p, sys.ld, sys.nt, &sys.nz, e->invdiag.p + fw.dsgn, e->invdiag.p + fw.linvT};
  return factor_solve_run(e, f, n, identity_rowmap(n, sys.ld).data(), m, B, X);
}

}  // extern "C"
