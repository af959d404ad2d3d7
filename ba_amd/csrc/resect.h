// Pose refinement (resection) with the landmarks held fixed: the rules.
// Host only: no HIP include; the kernel (k_resect.hip), hostcheck.cpp (ba_hostcheck_refine_poses) and, through the
// engine, the C++ class apply the same functions.
//
// With the landmarks fixed the problem is one 6-parameter least-squares problem per pose:
//   E_p = sum w |z - pi_cam(P)|^2   over EVERY projection residual whose measuring pose is p,
//   P = R_sw X + t_sw X[3],   T_sw = (T_wp T_vs)^-1 formed as k_pose_prep forms it (quaternion product renormalised),
//   X the landmark's homogeneous WORLD point (LmSize 3: lm_x[cur]; LmSize 1: lm_xw, current outside a Solve).
// The landmark is fixed in the world, so one expression serves LmSize 1 and 3: the LM == 3 branch of
// bad::proj_jacobians and its jm block.  With LmSize 1 an observation taken from the landmark's own reference pose
// counts like any other: the world point does not move with the pose here, so the observation does constrain it
// (k_linearize zeroes that block in the joint problem, where the point rides on its reference pose).  A landmark stored
// as a pure direction (X[3] = 0) is valid input and constrains the rotation only.
// NOT part of the cost: the pose's unary, binary and inertial residuals and its dense priors.  The active flags of poses
// and landmarks are not consulted: the id list decides.
//   weights    obs_w0; with huber_width > 0, w = w0 min(1, huber_width / sqrt(w0 |r|^2)) at every evaluated point
//   unknowns   the six parameters of k_apply_poses: t <- t - delta[0:3], q <- normalize(q exp(-delta[3:6])); velocities
//              and biases are not touched.  fixed_mask bit i: parameter i's row and column leave the system, delta_i is
//              exactly 0; bits 0-2 all set leave t bitwise, bits 3-5 all set leave q bitwise
//   iteration  H = sum w Jm^T Jm (21 unique), g = sum w Jm^T r, d = damp_clamp(diag H), (H + lambda diag d) delta = g,
//              predicted decrease delta^T (lambda D delta + g), gain ratio and Nielsen's rule of damping.h; the sums are
//              taken at the trial point, so an accepted step needs no second evaluation
//   cheirality an observation with P.z <= 0 or a non-finite P at the STARTING pose is excluded for the whole call and
//              counted; a trial pose that puts a used observation at depth <= 0 has E = +inf: rejected like an increase
//   stop       E == 0 at working precision (E <= F, the rounding floor of the cost defined below: a pose that its
//              observations determine exactly, 3 of them for 6 parameters, drives E to that floor, and every decision
//              taken below it would be taken on rounding noise), or c = max_i |g_i| / sqrt(H_ii E) <=
//              gradient_tolerance over the free parameters, or an accepted step with
//              |delta_t| <= step_tolerance (|t| + step_tolerance) and |delta_w| <= step_tolerance
//   status     in this order: TOO_FEW_OBSERVATIONS (2 used < free parameters; a pose without observations included);
//              FAILED (non-finite starting pose or cost: a pose that is not finite has no usable observation and
//              reports the former, a finite pose with a non-finite pixel or weight reports FAILED); then OK or
//              NOT_CONVERGED.  The first two leave the pose bit for bit; NOT_CONVERGED is written when the cost fell.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "damping.h"
#include "dmath.h"

// (small constant loops: unrolled in the kernel, so that every array below stays in registers)
#ifdef __HIPCC__
#define RS_UNROLL _Pragma("unroll")
#else
#define RS_UNROLL
#endif

namespace bae {

enum RsStatus { kRsOk = 0, kRsNotConverged, kRsTooFewObservations, kRsFailed, kRsStatusCount };
static const int kRsMaxIterations = 64;
static const int kRsResult = 8;   // status, used, iterations, cost at start, cost at end, smallest depth, c, excluded
// the sums: H unique (row-major upper), g (6), E, its rounding floor F
static const int kRsH = 21, kRsE = 27, kRsF = 28, kRsSums = 29;
static const int kRsRed = 32;     // one reduction row: the 29 sums, used count, smallest depth, 1 spare
// The rounding floor of the cost: a residual z - pi(P) is the difference of two numbers of the size of the pixel, formed
// through about eight roundings (rotate, translate, divide, scale, offset, subtract), so it carries an absolute error of
// up to about kRsFloorUlps eps |z| whatever the pose, and F = sum w (kRsFloorUlps eps)^2 |z|^2 is the cost of residuals
// that are nothing but that error.
static const double kRsFloorUlps = 8.0;

struct RsOptions {
  int max_iterations = 20, write_back = 1;
  unsigned fixed_mask = 0;
  double lambda0 = 1e-3, gradient_tolerance = 1e-6, step_tolerance = 1e-12, huber_width = 0.0;
};

BA_HD bool rs_finite(double v) { return v - v == 0.0; }
BA_HD double rs_inf() { return HUGE_VAL; }
BA_HD int rs_diag(int i) { return i * 6 - i * (i - 1) / 2; }   // index of H_ii among the unique entries
BA_HD int rs_free_count(unsigned mask) {
  int n = 0;
  RS_UNROLL
  for (int i = 0; i < 6; ++i) n += (mask >> i & 1u) ? 0 : 1;
  return n;
}

// T_wp and, for the camera mounted at tvs7 (t, q xyzw), T_sw = (T_wp T_vs)^-1: k_pose_prep's operations
BA_HD void rs_sensor(const double* pose7, const double* tvs7, bad::Rt* wp, bad::Rt* sw) {
  wp->R = bad::quat_to_rot(pose7[3], pose7[4], pose7[5], pose7[6]);
  wp->t = bad::v3(pose7[0], pose7[1], pose7[2]);
  const double qv[4] = {tvs7[3], tvs7[4], tvs7[5], tvs7[6]}, qp[4] = {pose7[3], pose7[4], pose7[5], pose7[6]};
  double q[4];
  bad::quat_mul(qp, qv, q);
  bad::quat_normalize(q);
  bad::Rt ws;
  ws.R = bad::quat_to_rot(q[0], q[1], q[2], q[3]);
  ws.t = bad::mul(wp->R, bad::v3(tvs7[0], tvs7[1], tvs7[2])) + wp->t;
  *sw = bad::inverse(ws);
}

// the point of an observation in its sensor; is the observation used (decided at the starting pose)?
BA_HD bad::V3 rs_point(const bad::Rt& t_sw, const double* X) {
  return bad::mul(t_sw.R, bad::v3(X[0], X[1], X[2])) + t_sw.t * X[3];
}
BA_HD bool rs_usable(bad::V3 P) { return rs_finite(P.x) && rs_finite(P.y) && rs_finite(P.z) && P.z > 0.0; }

// one used observation's share of [H | g | E] at the pose whose transforms are given; returns its depth.
// guard: a depth that is not > 0 makes E +inf
BA_HD double rs_eval(const bad::Cam& cam, const double* z, double w0, const double* X, const bad::Rt& t_wp,
                     const bad::Rt& t_sw, const bad::M3& R_sv, double huber, bool guard, double* v) {
  bad::Rt sv;
  sv.R = R_sv;
  sv.t = bad::v3(0.0, 0.0, 0.0);
  bad::ProjJac<3> J;
  bad::proj_jacobians<3>(cam, z, X, t_sw, sv, t_wp, sv, sv, sv, false, &J);
  const double depth = rs_point(t_sw, X).z;
  const double sq = J.r[0] * J.r[0] + J.r[1] * J.r[1];
  double w = w0;
  if (huber > 0.0) {
    const double en = sqrt(sq * w);
    if (en > huber) w *= huber / en;
  }
  int k = 0;
  RS_UNROLL
  for (int p = 0; p < 6; ++p)
    RS_UNROLL
    for (int c = p; c < 6; ++c) v[k++] = (J.jm[p] * J.jm[c] + J.jm[6 + p] * J.jm[6 + c]) * w;
  RS_UNROLL
  for (int p = 0; p < 6; ++p) v[kRsH + p] = (J.jm[p] * J.r[0] + J.jm[6 + p] * J.r[1]) * w;
  v[kRsE] = (guard && !(depth > 0.0)) ? rs_inf() : sq * w;
  const double ulp = kRsFloorUlps * 2.220446049250313e-16;
  v[kRsF] = (z[0] * z[0] + z[1] * z[1]) * (ulp * ulp) * w;
  return depth;
}

// fixed parameters leave the sums: their rows and columns of H and entries of g are zero
BA_HD void rs_mask_sums(double* s, unsigned mask) {
  if (!mask) return;
  int k = 0;
  RS_UNROLL
  for (int p = 0; p < 6; ++p)
    RS_UNROLL
    for (int c = p; c < 6; ++c, ++k)
      if ((mask >> p & 1u) || (mask >> c & 1u)) s[k] = 0.0;
  RS_UNROLL
  for (int p = 0; p < 6; ++p)
    if (mask >> p & 1u) s[kRsH + p] = 0.0;
}

// (H + lambda diag d) delta = g by LDL^T, unrolled; a fixed parameter has the unit row and delta exactly 0
BA_HD void rs_solve6(const double* s, const double* d, double lambda, unsigned mask, double* delta) {
  double A[6][6], D[6], y[6];
  int k = 0;
  RS_UNROLL
  for (int p = 0; p < 6; ++p)
    RS_UNROLL
    for (int c = p; c < 6; ++c, ++k) A[c][p] = s[k];
  RS_UNROLL
  for (int p = 0; p < 6; ++p) A[p][p] = (mask >> p & 1u) ? 1.0 : A[p][p] + lambda * d[p];
  RS_UNROLL
  for (int j = 0; j < 6; ++j) {
    double dj = A[j][j];
    RS_UNROLL
    for (int q = 0; q < j; ++q) dj -= A[j][q] * A[j][q] * D[q];
    D[j] = dj;
    const double inv = 1.0 / dj;
    RS_UNROLL
    for (int i = j + 1; i < 6; ++i) {
      double a = A[i][j];
      RS_UNROLL
      for (int q = 0; q < j; ++q) a -= A[i][q] * A[j][q] * D[q];
      A[i][j] = a * inv;
    }
  }
  RS_UNROLL
  for (int i = 0; i < 6; ++i) {
    double a = s[kRsH + i];
    RS_UNROLL
    for (int q = 0; q < i; ++q) a -= A[i][q] * y[q];
    y[i] = a;
  }
  RS_UNROLL
  for (int i = 5; i >= 0; --i) {
    double a = y[i] / D[i];
    RS_UNROLL
    for (int q = i + 1; q < 6; ++q) a -= A[q][i] * delta[q];
    delta[i] = (mask >> i & 1u) ? 0.0 : a;
  }
}

// x [+] (-delta) on the six parameters, as k_apply_poses
BA_HD void rs_apply(const double* pose7, const double* delta, unsigned mask, double* out7) {
  RS_UNROLL
  for (int i = 0; i < 3; ++i) out7[i] = pose7[i] - delta[i];
  if ((mask & 56u) == 56u) {
    RS_UNROLL
    for (int i = 3; i < 7; ++i) out7[i] = pose7[i];
    return;
  }
  double qe[4], q[4];
  bad::so3_exp(bad::v3(-delta[3], -delta[4], -delta[5]), qe);
  bad::quat_mul(pose7 + 3, qe, q);
  bad::quat_normalize(q);
  RS_UNROLL
  for (int i = 0; i < 4; ++i) out7[3 + i] = q[i];
}

// ---- one pose's refinement: what every thread of the pose's workgroup (the kernel) or the loop (the host) carries ----
struct RsPose {
  double x[7];              // the pose: t, q
  double cur[kRsSums];      // [H | g | E] at x, fixed rows and columns zero
  double delta[6], pred;    // the step being tried and its predicted decrease
  DampState ds;
  double e0, c, depth;
  unsigned used, excluded;
  int iterations, status;
  bool active;              // a trial pose is waiting for its sums
};

// convergence at the current point, or the next trial step
BA_HD void rs_continue(RsPose* m, const RsOptions& o) {
  const double E = m->cur[kRsE];
  double c = 0.0;
  if (E != 0.0)
    RS_UNROLL
    for (int i = 0; i < 6; ++i)
      if (!(o.fixed_mask >> i & 1u)) {
        const double ci = fabs(m->cur[kRsH + i]) / sqrt(m->cur[rs_diag(i)] * E);
        c = ci > c ? ci : c;
      }
  m->c = c;
  m->active = false;
  // (E <= F: the cost is zero as far as the residuals can tell; E == 0 is the case F == 0 of it)
  if (E <= m->cur[kRsF] || c <= o.gradient_tolerance) { m->status = kRsOk; return; }
  if (m->iterations >= o.max_iterations) { m->status = kRsNotConverged; return; }
  double d[6];
  RS_UNROLL
  for (int i = 0; i < 6; ++i) d[i] = (o.fixed_mask >> i & 1u) ? 0.0 : damp_clamp(m->cur[rs_diag(i)]);
  rs_solve6(m->cur, d, m->ds.lambda, o.fixed_mask, m->delta);
  double dDd = 0.0, pred = 0.0;
  RS_UNROLL
  for (int i = 0; i < 6; ++i) damp_term(m->delta[i], m->cur[kRsH + i], d[i], m->ds.lambda, &dDd, &pred);
  m->pred = pred;
  m->active = true;
}
// the starting pose with its sums (masked), used / excluded counts and smallest depth there
BA_HD void rs_begin(RsPose* m, const RsOptions& o, const double* pose7, const double* tot, unsigned used, unsigned excluded,
                    double depth) {
  bool fin = rs_finite(tot[kRsE]);
  RS_UNROLL
  for (int i = 0; i < 7; ++i) { m->x[i] = pose7[i]; fin = fin && rs_finite(pose7[i]); }
  RS_UNROLL
  for (int i = 0; i < kRsSums; ++i) m->cur[i] = tot[i];
  RS_UNROLL
  for (int i = 0; i < 6; ++i) m->delta[i] = 0.0;
  m->pred = 0.0;
  m->ds.lambda = o.lambda0; m->ds.nu = 2.0;
  m->e0 = tot[kRsE]; m->c = 0.0; m->depth = depth;
  m->used = used; m->excluded = excluded;
  m->iterations = 0;
  m->active = false;
  if (2 * (int)used < rs_free_count(o.fixed_mask)) m->status = kRsTooFewObservations;
  else if (!fin) m->status = kRsFailed;
  else rs_continue(m, o);
}
// the sums (masked) and smallest depth at the trial pose of an active pose: accept or reject, then rs_continue
BA_HD void rs_step(RsPose* m, const RsOptions& o, const double* trial7, const double* tot, double depth) {
  const double rho = damp_gain_ratio(m->cur[kRsE], tot[kRsE], m->pred);
  const bool accept = damp_update(&m->ds, rho);
  m->iterations += 1;
  if (accept) {
    RS_UNROLL
    for (int i = 0; i < 7; ++i) m->x[i] = trial7[i];
    RS_UNROLL
    for (int i = 0; i < kRsSums; ++i) m->cur[i] = tot[i];
    m->depth = depth;
    const double* dl = m->delta;
    const double dt = sqrt(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]);
    const double dw = sqrt(dl[3] * dl[3] + dl[4] * dl[4] + dl[5] * dl[5]);
    const double tn = sqrt(m->x[0] * m->x[0] + m->x[1] * m->x[1] + m->x[2] * m->x[2]);
    if (o.step_tolerance > 0.0 && dt <= o.step_tolerance * (tn + o.step_tolerance) && dw <= o.step_tolerance) {
      RsOptions stop = o;
      stop.max_iterations = 0;           // (only c of the accepted point is wanted)
      rs_continue(m, stop);
      m->status = kRsOk;
      m->active = false;
      return;
    }
  }
  rs_continue(m, o);
}
// is the pose arrived at the result?  One definition, for the refinement's own state and for a result row
BA_HD bool rs_accepted_values(int status, double e_start, double e_end) {
  if (status == kRsOk) return true;
  return status == kRsNotConverged && e_end < e_start;
}
BA_HD bool rs_accepted(const RsPose& m) { return rs_accepted_values(m.status, m.e0, m.cur[kRsE]); }
BA_HD bool rs_row_accepted(const double* r) { return rs_accepted_values((int)r[0], r[3], r[4]); }
BA_HD void rs_result(const RsPose& m, double* r) {
  const bool ran = m.status == kRsOk || m.status == kRsNotConverged;
  r[0] = m.status; r[1] = m.used; r[2] = m.iterations; r[3] = ran ? m.e0 : 0.0; r[4] = ran ? m.cur[kRsE] : 0.0;
  r[5] = m.used ? m.depth : 0.0; r[6] = m.c; r[7] = m.excluded;
}
// the undamped H at the end point, full symmetric, row-major (zero where the refinement did not run)
BA_HD void rs_info(const RsPose& m, double* h36) {
  const bool ran = m.status == kRsOk || m.status == kRsNotConverged;
  int k = 0;
  RS_UNROLL
  for (int p = 0; p < 6; ++p)
    RS_UNROLL
    for (int c = p; c < 6; ++c, ++k) h36[p * 6 + c] = h36[c * 6 + p] = ran ? m.cur[k] : 0.0;
}

// ---- the per-pose observation list -------------------------------------------------------------------------------
// CSR over ALL poses by pose id: idx[ptr[p] .. ptr[p + 1]) are the positions, ascending, in the engine's sorted
// observation order of the observations whose measuring pose is p.  A counting sort of obs_pose; indices only, so
// nothing in it goes stale when obs_z, obs_w0, obs_cam or the landmarks are uploaded again.
inline bool build_pose_obs_lists(uint32_t P, size_t O, const uint32_t* obs_pose, std::vector<uint32_t>* ptr,
                                 std::vector<uint32_t>* idx) {
  ptr->assign((size_t)P + 1, 0);
  idx->assign(O, 0);
  for (size_t s = 0; s < O; ++s) {
    if (obs_pose[s] >= P) return false;
    (*ptr)[obs_pose[s] + 1] += 1;
  }
  for (uint32_t p = 0; p < P; ++p) (*ptr)[p + 1] += (*ptr)[p];
  std::vector<uint32_t> at(ptr->begin(), ptr->end() - 1);
  for (size_t s = 0; s < O; ++s) (*idx)[at[obs_pose[s]]++] = (uint32_t)s;
  return true;
}

}  // namespace bae
