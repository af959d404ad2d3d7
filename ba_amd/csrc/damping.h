// Levenberg-Marquardt damping of the Gauss-Newton step: the rules, and their host restatement.
// Host only: no HIP include; the kernels (k_proj.hip, k_damp.hip), the C++ class and hostcheck.cpp
// (ba_hostcheck_damping) apply the same functions.
//
// H = J^T Lambda J is the full normal matrix of the last linearisation, g the right-hand side the step solves for.
// The damped step solves (H + lambda diag(d)) delta = g with d_j = clamp(H_jj) for every free parameter; a masked pose
// parameter keeps the reference's 1e6 and gets no damping (d_j = 0).  In the reduced form of the engine:
//   landmarks   V_lambda = V + lambda diag(d_l), d_l from diag(V) after the 1e-6 guard of invert_v; everything derived
//               from V^-1 uses V_lambda^-1 (factor rows, lm_vinv, the Schur part of S and of the rhs, back-substitution)
//   poses       S_jj += lambda clamp(U_jj) once S is complete, U_jj = S_jj - (Schur part)_jj the pose diagonal of H
//   predicted   E(0) - E_model(delta) = delta^T (lambda diag(d) delta + g), in the units of the error sums
//   control     Nielsen's rule on the gain ratio rho = (E_pre - E_post) / predicted
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>

#ifdef __HIPCC__
#define BA_DAMP_HD __host__ __device__
#else
#define BA_DAMP_HD
#endif

namespace bae {

static const double kDampDiagMin = 1e-6, kDampDiagMax = 1e32;     // clamp of the damping diagonal
static const double kDampLambdaMin = 1e-12, kDampLambdaMax = 1e12;  // lambda stays in this interval

// d_j = min(max(H_jj, 1e-6), 1e32)
BA_DAMP_HD inline double damp_clamp(double h_jj) {
  const double lo = h_jj > kDampDiagMin ? h_jj : kDampDiagMin;
  return lo < kDampDiagMax ? lo : kDampDiagMax;
}

// The 1e-6 guard of invert_v (BundleAdjuster.cpp:431-440) and the damping of the unique entries Vs of V
// (00 | 00 01 02 11 12 22), in place: d_l = clamp(diag V) after the guard, V_ii += lambda d_l[i].  The guard of
// invert_v does not fire again on the result: every diagonal entry is then at least 1e-6 (1 + lambda).
template <int LM>
BA_DAMP_HD inline void damp_v(double* Vs, double lambda, double* dl) {
  if constexpr (LM == 1) {
    double v = Vs[0];
    if (fabs(v) < 1e-6) v += 1e-6;
    dl[0] = damp_clamp(v);
    Vs[0] = v + lambda * dl[0];
  } else {
    const double a = Vs[0], b = Vs[1], c = Vs[2], ee = Vs[3], f = Vs[4], i = Vs[5];
    const double nrm = a * a + ee * ee + i * i + 2.0 * (b * b + c * c + f * f);
    const double g = sqrt(nrm) < 1e-6 ? 1e-6 : 0.0;
    const double v0 = a + g, v1 = ee + g, v2 = i + g;
    dl[0] = damp_clamp(v0); dl[1] = damp_clamp(v1); dl[2] = damp_clamp(v2);
    Vs[0] = v0 + lambda * dl[0]; Vs[3] = v1 + lambda * dl[1]; Vs[5] = v2 + lambda * dl[2];
  }
}

// d_p of one unmasked pose parameter from the complete S and the Schur part of its diagonal
BA_DAMP_HD inline double damp_pose_diag(double s_jj, double schur_jj) { return damp_clamp(s_jj - schur_jj); }

// one parameter's share of delta^T D delta and of the predicted decrease delta^T (lambda D delta + g)
BA_DAMP_HD inline void damp_term(double delta, double g, double d, double lambda, double* dDd, double* pred) {
  const double q = d * delta * delta;
  *dDd += q;
  *pred += lambda * q + delta * g;
}

// ---- control on the host (Nielsen's rule) --------------------------------------------------------------------------
struct DampState {
  double lambda, nu;
};
// (std::max and std::min written out, operand for operand, so that the kernels of k_triang.hip can apply the rule too)
BA_DAMP_HD inline double damp_keep_lambda(double lambda) {
  const double lo = lambda < kDampLambdaMin ? kDampLambdaMin : lambda;
  return kDampLambdaMax < lo ? kDampLambdaMax : lo;
}
BA_DAMP_HD inline double damp_gain_ratio(double e_pre, double e_post, double predicted) { return (e_pre - e_post) / predicted; }
// Returns whether the step is accepted.  Accepted (rho > 0): lambda <- lambda max(1/3, 1 - (2 rho - 1)^3), nu <- 2;
// otherwise (a NaN ratio included) lambda <- lambda nu, nu <- 2 nu.
BA_DAMP_HD inline bool damp_update(DampState* s, double rho) {
  const bool accept = rho > 0.0;
  if (accept) {
    const double t = 2.0 * rho - 1.0, third = 1.0 / 3.0, cube = 1.0 - t * t * t;
    s->lambda = damp_keep_lambda(s->lambda * (third < cube ? cube : third));
    s->nu = 2.0;
  } else {
    s->lambda = damp_keep_lambda(s->lambda * s->nu);
    s->nu *= 2.0;
  }
  return accept;
}

// ---- host restatement of the sums of k_damp_terms: n parameters with step, right-hand side and damping diagonal ------
inline void damp_terms_host(size_t n, const double* delta, const double* g, const double* d, double lambda, double* dDd,
                            double* pred) {
  *dDd = 0.0;
  *pred = 0.0;
  for (size_t j = 0; j < n; ++j) damp_term(delta[j], g[j], d[j], lambda, dDd, pred);
}

}  // namespace bae
