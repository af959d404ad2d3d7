// Landmark triangulation and per-landmark refinement with the poses held fixed: the rules.
// Host only: no HIP include; the kernel (k_triang.hip), hostcheck.cpp (ba_hostcheck_triangulate) and, through the
// engine, the C++ class apply the same functions.
//
// With the poses fixed the problem is one least-squares problem per landmark over its own parameters: the world point
// (LmSize 3) or the inverse depth rho along the ray of the reference sensor (LmSize 1).  Every observation is held as
//   P = T.R xv + T.t rho,   z ~ pi(P)
// with, LmSize 3, T = T_sw of the measuring sensor, xv the world point and rho the fourth coordinate held (1 after the
// linear estimate); LmSize 1, T = T_sw_m T_ws_r, xv = unit(T_sw_r x_w) the reference ray (k_world_to_sensor; a
// landmark uploaded as a pure direction, w = 0, is valid input) and rho the unknown.  The frame of xv (the world, or the
// reference sensor) is the landmark's frame below.
//   first      LmSize 3: the first observation; LmSize 1: the reference sensor itself (centre 0, bearing xv)
//   centre     c_a = -T.R^T T.t and bearing d_a = T.R^T unit(unproject(z_a)) of an observation, in the landmark's frame
//   baseline   max_a |c_a - c_first|; a landmark with fewer than 2 observations, or with
//              baseline^2 <= kTriBaselineRel^2 (1 + |c_first|^2), has TOO_FEW_VIEWS
//   parallax   max_a angle(d_first, d_a): O(k), and at least half the largest pairwise angle
//   linear     LmSize 3: X = (sum w (I - d d^T))^-1 sum w (I - d d^T) c, stored as [X, 1]
//              LmSize 1: rho = -sum w (b x R xv).(b x t) / sum w |b x t|^2,  b = unit(unproject(z)), (R, t) = T
//   refine     Levenberg-Marquardt on E = sum w |z - pi(P)|^2: V = sum w Jl^T Jl, b_l = sum w Jl^T r with the jl of
//              proj_jacobians; d = damp_clamp(diag V), (V + lambda diag d) delta = b_l, x <- x - delta; predicted
//              decrease delta^T (lambda D delta + b_l), gain ratio and Nielsen's rule of damping.h.  A trial point at
//              depth <= 0 in an observing sensor has E = +inf: rejected like a cost increase.  With huber_width > 0
//              w = w0 min(1, huber_width / sqrt(w0 |r|^2)) at every evaluated point.
//   stop       converged when E == 0, or c = max_i |b_i| / sqrt(V_ii E) <= gradient_tolerance (the cosine between the
//              residual and a Jacobian column, MINPACK's gtol), or an accepted |delta| <= step_tolerance (|x| + step_tolerance)
//   depth      P.z in the observing sensor, what the projection divides by (LmSize 1: of the point scaled by rho)
//   status     in this order: TOO_FEW_VIEWS; FAILED (a non-finite starting point, cost or depth); LOW_PARALLAX
//              (parallax < min_parallax); BEHIND_CAMERA (smallest depth <= 0 at the starting point); then OK or
//              NOT_CONVERGED from the refinement.  The last four leave the coordinates as they were.  NOT_CONVERGED
//              is written when the cost fell; with linear_init the linear estimate is itself a result (it is what
//              max_iterations = 0 returns), so it is written when the cost did not rise, which rejected steps ensure.
#pragma once
#include <cmath>

#include "damping.h"
#include "dmath.h"

namespace bae {

enum TriStatus { kTriOk = 0, kTriNotConverged, kTriTooFewViews, kTriLowParallax, kTriBehindCamera, kTriFailed, kTriStatusCount };
static const int kTriMaxIterations = 64;
static const double kTriBaselineRel = 1e-12;
static const int kTriResult = 8;   // status, observations, iterations, cost at start, cost at end, parallax, smallest depth, c

struct TriOptions {
  int linear_init = 1, max_iterations = 20, write_back = 1;
  double lambda0 = 1e-3, gradient_tolerance = 1e-6, step_tolerance = 1e-12, min_parallax = 0.0, huber_width = 0.0;
};

struct TriObs {
  bad::Rt T;
  bad::Cam cam;
  double z[2], w0;
};

template <int LM>
struct TriSums {
  static constexpr int NV = LM * (LM + 1) / 2, N = NV + LM + 1;   // V unique (00 | 00 01 02 11 12 22), b_l, E
  static constexpr int NL = LM == 3 ? 9 : 2;                      // the sums of the linear estimate
};

BA_HD bool tri_finite(double v) { return v - v == 0.0; }
BA_HD double tri_max(double a, double b) { return b > a ? b : a; }
BA_HD double tri_min(double a, double b) { return b < a ? b : a; }
BA_HD double tri_inf() { return HUGE_VAL; }

// the landmark in its frame from the coordinates held: LmSize 3 (xv, rho) = x_w itself; LmSize 1 the ray and inverse
// depth of k_world_to_sensor in the reference sensor T_sw_r
template <int LM>
BA_HD void tri_held(const double* x_w, const bad::Rt& t_sw_r, double* xv, double* rho) {
  if (LM == 1) {
    const bad::V3 p = bad::mul(t_sw_r.R, bad::v3(x_w[0], x_w[1], x_w[2])) + t_sw_r.t * x_w[3];
    const double len = sqrt(bad::dot(p, p));
    xv[0] = p.x / len; xv[1] = p.y / len; xv[2] = p.z / len;
    *rho = x_w[3] / len;
  } else {
    xv[0] = x_w[0]; xv[1] = x_w[1]; xv[2] = x_w[2];
    *rho = x_w[3];
  }
}
// ... and back to world coordinates (LmSize 1: k_sensor_to_world in the reference sensor T_ws_r)
template <int LM>
BA_HD void tri_world(const double* xv, double rho, const bad::Rt& t_ws_r, double* x_w) {
  if (LM == 1) {
    const bad::V3 p = bad::mul(t_ws_r.R, bad::v3(xv[0], xv[1], xv[2])) + t_ws_r.t * rho;
    x_w[0] = p.x; x_w[1] = p.y; x_w[2] = p.z; x_w[3] = rho;
  } else {
    x_w[0] = xv[0]; x_w[1] = xv[1]; x_w[2] = xv[2]; x_w[3] = rho;
  }
}

// centre and unit bearing of an observation in the landmark's frame
BA_HD void tri_centre_bearing(const TriObs& o, bad::V3* c, bad::V3* d) {
  *c = bad::mulT(o.T.R, o.T.t) * -1.0;
  const bad::V3 u = bad::unproject(o.cam, o.z[0], o.z[1]);
  const bad::V3 b = u * (1.0 / sqrt(bad::dot(u, u)));
  *d = bad::mulT(o.T.R, b);
}
// angle between two unit bearings; squared distance of two centres
BA_HD double tri_angle(bad::V3 d0, bad::V3 d) {
  const bad::V3 x = bad::cross(d0, d);
  return atan2(sqrt(bad::dot(x, x)), bad::dot(d0, d));
}
BA_HD double tri_dist2(bad::V3 c0, bad::V3 c) {
  const bad::V3 x = c - c0;
  return bad::dot(x, x);
}

// one observation's share of the sums of the linear estimate
template <int LM>
BA_HD void tri_linear_terms(const TriObs& o, const double* xv, double* v) {
  const double w = o.w0;
  if (LM == 3) {
    bad::V3 c, d;
    tri_centre_bearing(o, &c, &d);
    v[0] = w * (1.0 - d.x * d.x); v[1] = -w * d.x * d.y; v[2] = -w * d.x * d.z;
    v[3] = w * (1.0 - d.y * d.y); v[4] = -w * d.y * d.z; v[5] = w * (1.0 - d.z * d.z);
    const double dc = bad::dot(d, c);
    v[6] = w * (c.x - d.x * dc); v[7] = w * (c.y - d.y * dc); v[8] = w * (c.z - d.z * dc);
  } else {
    const bad::V3 u = bad::unproject(o.cam, o.z[0], o.z[1]);
    const bad::V3 b = u * (1.0 / sqrt(bad::dot(u, u)));
    const bad::V3 br = bad::cross(b, bad::mul(o.T.R, bad::v3(xv[0], xv[1], xv[2]))), bt = bad::cross(b, o.T.t);
    v[0] = w * bad::dot(br, bt);
    v[1] = w * bad::dot(bt, bt);
  }
}
// symmetric 3 x 3 solve by cofactors, s = the unique entries (00 01 02 11 12 22)
BA_HD void tri_solve3(const double* s, const double* r, double* x) {
  const double a = s[0], b = s[1], c = s[2], e = s[3], f = s[4], i = s[5];
  const double A00 = e * i - f * f, A01 = c * f - b * i, A02 = b * f - c * e;
  const double A11 = a * i - c * c, A12 = b * c - a * f, A22 = a * e - b * b;
  const double id = 1.0 / (a * A00 + b * A01 + c * A02);
  x[0] = (A00 * r[0] + A01 * r[1] + A02 * r[2]) * id;
  x[1] = (A01 * r[0] + A11 * r[1] + A12 * r[2]) * id;
  x[2] = (A02 * r[0] + A12 * r[1] + A22 * r[2]) * id;
}
// the linear estimate from the summed terms: the landmark's parameters (LmSize 3: xv, rho = 1; LmSize 1: rho)
template <int LM>
BA_HD void tri_linear_solve(const double* tot, double* xv, double* rho) {
  if (LM == 3) {
    tri_solve3(tot, tot + 6, xv);
    *rho = 1.0;
  } else {
    *rho = -tot[0] / tot[1];
  }
}

// depth of P in the sensor of an observation: what the projection divides by.  LmSize 1: P is the point scaled by rho;
// the sign of rho itself is not judged here (k_apply_landmarks keeps its own guard on it)
template <int LM>
BA_HD double tri_depth(const TriObs& o, const double* xv, double rho) {
  return o.T.R.m[6] * xv[0] + o.T.R.m[7] * xv[1] + o.T.R.m[8] * xv[2] + o.T.t.z * rho;
}
// one observation's share of [V | b_l | E] at (xv, rho); returns its depth.  guard: a depth that is not > 0 makes E +inf
template <int LM>
BA_HD double tri_eval(const TriObs& o, const double* xv, double rho, double huber, bool guard, double* v) {
  constexpr int NV = TriSums<LM>::NV;
  const double x[4] = {xv[0], xv[1], xv[2], rho};
  bad::Rt I;
  for (int k = 0; k < 9; ++k) I.R.m[k] = (k % 4 == 0) ? 1.0 : 0.0;
  I.t = bad::v3(0.0, 0.0, 0.0);
  bad::ProjJac<LM> J;
  bad::proj_jacobians<LM>(o.cam, o.z, x, o.T, I, I, I, I, I, true, &J);
  const double depth = tri_depth<LM>(o, xv, rho);
  const double sq = J.r[0] * J.r[0] + J.r[1] * J.r[1];
  double w = o.w0;
  if (huber > 0.0) {
    const double en = sqrt(sq * w);
    if (en > huber) w *= huber / en;
  }
  int k = 0;
  for (int p = 0; p < LM; ++p)
    for (int c = p; c < LM; ++c) v[k++] = (J.jl[p] * J.jl[c] + J.jl[LM + p] * J.jl[LM + c]) * w;
  for (int p = 0; p < LM; ++p) v[NV + p] = (J.jl[p] * J.r[0] + J.jl[LM + p] * J.r[1]) * w;
  v[NV + LM] = (guard && !(depth > 0.0)) ? tri_inf() : sq * w;
  return depth;
}

// ---- one landmark's refinement: what every lane of the landmark (the kernel) or the loop (the host) carries ----------
template <int LM>
struct TriLm {
  double x[LM];                       // the parameters: world point | inverse depth
  double cur[TriSums<LM>::N];         // [V | b_l | E] at x
  double delta[LM], pred;             // the step being tried and its predicted decrease
  DampState ds;
  double e0, c, parallax, depth;
  int iterations, status;
  bool active;                        // a trial point is waiting for its sums
};

template <int LM>
BA_HD double tri_diag(const double* s, int i) { return LM == 1 ? s[0] : s[i == 0 ? 0 : i == 1 ? 3 : 5]; }

// convergence at the current point, or the next trial step
template <int LM>
BA_HD void tri_continue(TriLm<LM>* m, const TriOptions& o) {
  constexpr int NV = TriSums<LM>::NV;
  const double E = m->cur[NV + LM];
  double c = 0.0;
  if (E != 0.0)
    for (int i = 0; i < LM; ++i) c = tri_max(c, fabs(m->cur[NV + i]) / sqrt(tri_diag<LM>(m->cur, i) * E));
  m->c = c;
  m->active = false;
  if (E == 0.0 || c <= o.gradient_tolerance) { m->status = kTriOk; return; }
  if (m->iterations >= o.max_iterations) { m->status = kTriNotConverged; return; }
  double d[LM], s[NV];
  for (int i = 0; i < NV; ++i) s[i] = m->cur[i];
  for (int i = 0; i < LM; ++i) d[i] = damp_clamp(tri_diag<LM>(m->cur, i));
  if (LM == 1) {
    s[0] += m->ds.lambda * d[0];
    m->delta[0] = m->cur[NV] / s[0];
  } else {
    s[0] += m->ds.lambda * d[0]; s[3] += m->ds.lambda * d[1]; s[5] += m->ds.lambda * d[2];
    tri_solve3(s, m->cur + NV, m->delta);
  }
  double dDd = 0.0, pred = 0.0;
  for (int i = 0; i < LM; ++i) damp_term(m->delta[i], m->cur[NV + i], d[i], m->ds.lambda, &dDd, &pred);
  m->pred = pred;
  m->active = true;
}
// the trial point of an active landmark
template <int LM>
BA_HD void tri_trial(const TriLm<LM>& m, const double* xv, double rho, double* txv, double* trho) {
  if (LM == 3) {
    for (int i = 0; i < 3; ++i) txv[i] = m.x[i] - m.delta[i];
    *trho = rho;
  } else {
    for (int i = 0; i < 3; ++i) txv[i] = xv[i];
    *trho = m.x[0] - m.delta[0];
  }
}
// the starting point with its sums, the smallest depth there, parallax and baseline^2, |c_first|^2, k observations
template <int LM>
BA_HD void tri_begin(TriLm<LM>* m, const TriOptions& o, const double* x0, const double* tot, double depth, double parallax,
                     double base2, double c02, unsigned k) {
  constexpr int N = TriSums<LM>::N;
  bool fin = tri_finite(tot[N - 1]) && tri_finite(depth);
  for (int i = 0; i < LM; ++i) { m->x[i] = x0[i]; m->delta[i] = 0.0; fin = fin && tri_finite(x0[i]); }
  for (int i = 0; i < N; ++i) m->cur[i] = tot[i];
  m->pred = 0.0;
  m->ds.lambda = o.lambda0; m->ds.nu = 2.0;
  m->e0 = tot[N - 1]; m->c = 0.0; m->parallax = parallax; m->depth = depth;
  m->iterations = 0;
  m->active = false;
  if (k < 2 || base2 <= kTriBaselineRel * kTriBaselineRel * (1.0 + c02)) m->status = kTriTooFewViews;
  else if (!fin) m->status = kTriFailed;
  else if (parallax < o.min_parallax) m->status = kTriLowParallax;
  else if (depth <= 0.0) m->status = kTriBehindCamera;
  else tri_continue<LM>(m, o);
}
// the sums at the trial point of an active landmark: accept or reject, then tri_continue
template <int LM>
BA_HD void tri_step(TriLm<LM>* m, const TriOptions& o, const double* tot) {
  constexpr int N = TriSums<LM>::N;
  const double rho = damp_gain_ratio(m->cur[N - 1], tot[N - 1], m->pred);
  const bool accept = damp_update(&m->ds, rho);
  m->iterations += 1;
  if (accept) {
    double d2 = 0.0, x2 = 0.0;
    for (int i = 0; i < LM; ++i) { m->x[i] -= m->delta[i]; d2 += m->delta[i] * m->delta[i]; x2 += m->x[i] * m->x[i]; }
    for (int i = 0; i < N; ++i) m->cur[i] = tot[i];
    if (o.step_tolerance > 0.0 && sqrt(d2) <= o.step_tolerance * (sqrt(x2) + o.step_tolerance)) {
      TriOptions stop = o;
      stop.max_iterations = 0;           // (only c of the accepted point is wanted)
      tri_continue<LM>(m, stop);
      m->status = kTriOk;
      m->active = false;
      return;
    }
  }
  tri_continue<LM>(m, o);
}
// are the new coordinates written?
template <int LM>
BA_HD bool tri_accepted(const TriLm<LM>& m, const TriOptions& o) {
  constexpr int N = TriSums<LM>::N;
  if (m.status == kTriOk) return true;
  if (m.status != kTriNotConverged) return false;
  return o.linear_init ? m.cur[N - 1] <= m.e0 : m.cur[N - 1] < m.e0;
}
template <int LM>
BA_HD void tri_result(const TriLm<LM>& m, unsigned k, double depth_end, double* r) {
  constexpr int N = TriSums<LM>::N;
  r[0] = m.status; r[1] = k; r[2] = m.iterations; r[3] = m.e0; r[4] = m.cur[N - 1]; r[5] = m.parallax; r[6] = depth_end; r[7] = m.c;
}
// a landmark without observations
BA_HD void tri_result_none(double* r) {
  r[0] = kTriTooFewViews;
  for (int i = 1; i < kTriResult; ++i) r[i] = 0.0;
}

}  // namespace bae
