// Joint covariance of a mixed set of poses, calibration and landmarks (ba_hip_get_joint_state_marginals): the
// landmark columns of the right-hand side that k_jointcov.hip's substitution starts from, and V^-1 on the
// diagonal landmark blocks.  Plain C++17, no HIP; the per-entry arithmetic is shared with the device
// (k_jointcov.hip: k_joint_seed, k_joint_rhs, k_joint_lmdiag), the rest restates it for the CPU suite
// (hostcheck.cpp: ba_hostcheck_joint_state, tests/test_joint_state_plan.py).
//
// Full system [[U, W], [W^T, V]], S = U - W V^-1 W^T.  For the columns B = [E | b] with
//   b_{l,k} = -(W_l V_l^-1)[:, k]      (six entries per valid incidence of l, K at the calibration rows)
// the block of the inverse over the requested parameters is
//   B^T S^-1 B  +  V_l^-1 on the diagonal block of every requested landmark l:
//   Cov(p, l) = -Sigma_pp W_l V_l^-1,  Cov(l, l') = V_l^-1 W_l^T Sigma_pp W_l' V_l'^-1 (+ V_l^-1 when l = l').
// The incidences of a landmark and their order are those of lm_entry.h: the listed observations with an active
// pose, then (LM == 1) the reference-pose row W_r, then the calibration row E_l.  Incidences that hit the same six
// rows (duplicate observations) add, in that order.  A landmark without observations has no incidence: its column
// is zero and its V^-1 is 1e6 I (the guard of invert_v on a zero V).
#pragma once
#include <stdint.h>

#include <math.h>

#include <vector>

#include "jointcov.h"

#ifdef __HIPCC__
#define BAE_JS_FN __host__ __device__ __forceinline__
#else
#define BAE_JS_FN inline
#endif

namespace bae {

// V^-1 of landmark l as the landmark blocks read it (lm_sigma, k_selinv.hip): the linearisation's inverse, or
// 1e6 I for a landmark without observations, which no linearisation range covers
template <int LM>
BAE_JS_FN void joint_lm_vinv(uint32_t nobs, const double* vinv_l, double* Vi) {
  for (int a = 0; a < LM * LM; ++a) Vi[a] = nobs ? vinv_l[a] : (a % (LM + 1) == 0 ? 1e6 : 0.0);
}

// entry (i, k) of the column block of one incidence: -(W_e V^-1)[i][k] = -sum_c W_e[c][i] V^-1[c][k], w[c * 6 + i]
template <int LM>
BAE_JS_FN double joint_lm_value(const double* w, const double* Vi, int i, int k) {
  double s = 0.0;
  for (int c = 0; c < LM; ++c) s += w[c * 6 + i] * Vi[c * LM + k];
  return -s;
}

// ---- host restatement -------------------------------------------------------------------------------------
// the guard and closed-form inverse of k_linearize's invert_v, on the full symmetric V (row-major LM x LM)
template <int LM>
inline void joint_invert_v_host(const double* V, double* Vi) {
  if (LM == 1) {
    double v = V[0];
    if (fabs(v) < 1e-6) v += 1e-6;
    Vi[0] = 1.0 / v;
    return;
  }
  double a = V[0], b = V[1], c = V[2], e = V[4], f = V[5], i = V[8];
  const double nrm = a * a + e * e + i * i + 2.0 * (b * b + c * c + f * f);
  if (sqrt(nrm) < 1e-6) { a += 1e-6; e += 1e-6; i += 1e-6; }
  const double A00 = e * i - f * f, A01 = c * f - b * i, A02 = b * f - c * e;
  const double A11 = a * i - c * c, A12 = c * b - a * f, A22 = a * e - b * b;
  const double id = 1.0 / (a * A00 + b * A01 + c * A02);
  Vi[0] = A00 * id; Vi[1] = A01 * id; Vi[2] = A02 * id;
  Vi[3] = A01 * id; Vi[4] = A11 * id; Vi[5] = A12 * id;
  Vi[6] = A02 * id; Vi[7] = A12 * id; Vi[8] = A22 * id;
}

// The device's inputs, on the host.  Observations are in sorted order (by landmark).
struct JointStateHostIn {
  int LM = 1, D = 6, K = 0;
  uint32_t L = 0, O = 0, np = 0, lrow_base = 0;
  const uint32_t *lm_ptr = nullptr, *obs_pose = nullptr, *lm_ref_pose = nullptr;
  const int32_t* pose_opt = nullptr;
  const double* frow = nullptr;     // factor rows (structure.h)
  const double* crow = nullptr;     // [2 O + L][6]: E_l at 2 O + l; null without calibration
  const double* lm_vinv = nullptr;  // [L][LM LM]
};

// variant 0: the formula.  Deliberately wrong ones, which the CPU suite must tell from it: 1 leaves V^-1 off the
// diagonal landmark blocks, 2 drops the reference-pose incidence W_r (LM == 1), 3 gives the landmark columns the
// wrong sign.
//
// The entries of the columns c0 + LM q + k of the landmarks lms[q] (active, checked by the caller), appended to
// `ent` in the device's order; *incidences: the valid incidences walked.
template <int LM>
inline void joint_state_columns_host_lm(const JointStateHostIn& in, uint32_t n_lm, const uint32_t* lms, uint32_t c0,
                                        int variant, std::vector<JointEntry>& ent, uint64_t* incidences) {
  const int R = LM == 1 ? 6 : 8, WO = LM == 1 ? 4 : 2;
  uint64_t inc = 0;
  for (uint32_t q = 0; q < n_lm; ++q) {
    const uint32_t l = lms[q], a0 = in.lm_ptr[l], nobs = in.lm_ptr[l + 1] - a0, rp = in.lm_ref_pose[l];
    if (!nobs) continue;
    double Vi[LM * LM];
    joint_lm_vinv<LM>(nobs, in.lm_vinv + (size_t)l * LM * LM, Vi);
    bool any_listed = false;
    for (uint32_t e = 0; e < nobs; ++e) any_listed = any_listed || (LM == 1 && in.obs_pose[a0 + e] != rp);
    const uint32_t ne = nobs + (LM == 1 ? 1u : 0u) + (in.K > 0 ? 1u : 0u);
    for (uint32_t e = 0; e < ne; ++e) {
      bool valid;
      uint32_t base;
      int width;
      const double* w;
      if (e < nobs) {
        const uint32_t pm = in.obs_pose[a0 + e];
        const int po = in.pose_opt[pm];
        valid = !(LM == 1 && pm == rp) && po >= 0;
        base = po >= 0 ? (uint32_t)po * in.D : 0;
        width = 6;
        w = in.frow + ((size_t)(a0 + e) * R + WO) * 6;
      } else if (LM == 1 && e == nobs) {
        const int po = in.pose_opt[rp];
        valid = any_listed && po >= 0 && variant != 2;
        base = po >= 0 ? (uint32_t)po * in.D : 0;
        width = 6;
        w = in.frow + ((size_t)in.lrow_base + 2 * (size_t)l) * 6;
      } else {
        valid = in.K > 0 && in.crow;
        base = in.np;
        width = in.K;
        w = in.crow ? in.crow + (2 * (size_t)in.O + l) * 6 : nullptr;
      }
      if (!valid) continue;
      ++inc;
      for (int i = 0; i < width; ++i)
        for (int k = 0; k < LM; ++k) {
          const double v = joint_lm_value<LM>(w, Vi, i, k);
          ent.push_back({base + (uint32_t)i, c0 + (uint32_t)LM * q + (uint32_t)k, variant == 3 ? -v : v});
        }
    }
  }
  if (incidences) *incidences = inc;
}

inline void joint_state_columns_host(const JointStateHostIn& in, uint32_t n_lm, const uint32_t* lms, uint32_t c0,
                                     int variant, std::vector<JointEntry>& ent, uint64_t* incidences) {
  if (in.LM == 1) joint_state_columns_host_lm<1>(in, n_lm, lms, c0, variant, ent, incidences);
  else joint_state_columns_host_lm<3>(in, n_lm, lms, c0, variant, ent, incidences);
}

// k_joint_lmdiag: V^-1 added to the diagonal landmark blocks of cov (M x M); the lower entry goes to both halves
template <int LM>
inline void joint_state_add_vinv_lm(const JointStateHostIn& in, uint32_t n_lm, const uint32_t* lms, uint32_t c0, uint32_t M,
                                    double* cov) {
  for (uint32_t q = 0; q < n_lm; ++q) {
    const uint32_t l = lms[q], nobs = in.lm_ptr[l + 1] - in.lm_ptr[l];
    double Vi[LM * LM];
    joint_lm_vinv<LM>(nobs, in.lm_vinv + (size_t)l * LM * LM, Vi);
    for (int a = 0; a < LM; ++a)
      for (int b = 0; b <= a; ++b) {
        const size_t r = c0 + (size_t)LM * q + a, c = c0 + (size_t)LM * q + b;
        const double s = cov[r * M + c] + Vi[a * LM + b];
        cov[r * M + c] = cov[c * M + r] = s;
      }
  }
}

inline void joint_state_add_vinv(const JointStateHostIn& in, uint32_t n_lm, const uint32_t* lms, uint32_t c0, uint32_t M,
                                 double* cov) {
  if (in.LM == 1) joint_state_add_vinv_lm<1>(in, n_lm, lms, c0, M, cov);
  else joint_state_add_vinv_lm<3>(in, n_lm, lms, c0, M, cov);
}

}  // namespace bae
