// Leverages of projection residuals (ba_hip_get_projection_leverages, k_lever.hip): the 2 x 2 diagonal blocks
// H_aa of the hat matrix J (J^T J)^-1 J^T of the whitened Jacobian, from what a direct solve leaves behind.
// Plain C++17, no HIP: the plan (positions of requested ids, block-read count) serves the engine, and
// leverage_host restates the device formula over a dense Sigma for the CPU suite (hostcheck.cpp:
// ba_hostcheck_leverages, tests/test_leverages.py).
//
// Residual a of landmark l, measured from pose m, reference pose r (LM == 1): J_a = [A_a | B_a],
//   A_a   sqrt(w) dz_dx_meas at m, sqrt(w) dz_dx_ref at r, sqrt(w) dz_dk at the calibration columns
//   B_a   sqrt(w) dz_dlm
//   H_aa = A Sigma A^T - sym2((sum_f A_f t_f) V^-1 B^T) + B Sigma_ll B^T,   f in {m, r, k}
//   t_f      = sum_e Sigma_{p_f p_e} W_e           over the incidences e of l (lm_entry.h: listed observations
//                                                  with an active pose, the reference row W_r, E_l)
//   Sigma_ll = V^-1 + V^-1 (sum_f W_f^T t_f) V^-1   (the landmark marginal of k_selinv.hip)
// V^-1 enters through the Cholesky factor of V = sum_a B_a^T B_a (re-formed from obs_jl, with the guard of
// k_linearize's invert_v), V = L L^T, Li = L^-1:  M = B Li^T, N = (sum_f A_f t_f) Li^T, Q = I + Li U Li^T,
//   H_aa = A Sigma A^T - (N M^T + M N^T) + M Q M^T.
// The explicit inverse lm_vinv (cofactors) carries an error of eps cond(V) |V^-1| without structure, which
// B V^-1 B^T amplifies by another cond(V): 3e-10 at cond(V) = 2e4, against 1e-12 through the factor.
// Listing rule: an observation of an LM == 1 landmark from its own reference pose carries no pose block (it is
// no incidence either); a block of an inactive pose is absent; an inactive landmark drops B and every t_f.
#pragma once
#include <stdint.h>

#include <math.h>

#include <algorithm>
#include <vector>

#ifdef __HIPCC__
#define BAE_LEVER_FN __host__ __device__ __forceinline__
#else
#define BAE_LEVER_FN inline
#endif

namespace bae {

// Li = L^-1 for V = L L^T (row-major LM x LM, symmetric), after the guard of invert_v (k_proj.hip): a V below 1e-6
// gets 1e-6 on its diagonal.  A pivot that is not positive (a numerically singular V, which the explicit inverse
// does not survive either) is replaced by 1e-6.
template <int LM>
BAE_LEVER_FN void lever_factor(const double (&Vin)[LM][LM], double (&Li)[LM][LM]) {
  double V[LM][LM], L[LM][LM];
  double nrm = 0.0;
  for (int a = 0; a < LM; ++a)
    for (int b = 0; b < LM; ++b) { V[a][b] = Vin[a][b]; nrm += Vin[a][b] * Vin[a][b]; L[a][b] = 0.0; Li[a][b] = 0.0; }
  if (sqrt(nrm) < 1e-6)
    for (int a = 0; a < LM; ++a) V[a][a] += 1e-6;
  for (int j = 0; j < LM; ++j) {
    double d = V[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0)) d = 1e-6;
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < LM; ++i) {
      double x = V[i][j];
      for (int k = 0; k < j; ++k) x -= L[i][k] * L[j][k];
      L[i][j] = x / L[j][j];
    }
  }
  for (int c = 0; c < LM; ++c)      // column c of L^-1 by forward substitution
    for (int i = c; i < LM; ++i) {
      double x = i == c ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) x -= L[i][k] * Li[k][c];
      Li[i][c] = x / L[i][i];
    }
}

// sorted position (observations sorted by landmark, structure.h) of every residual id
inline void lever_positions(const std::vector<uint32_t>& obs_perm, std::vector<uint32_t>& pos_of_rid) {
  pos_of_rid.assign(obs_perm.size(), 0);
  for (uint32_t s = 0; s < obs_perm.size(); ++s) pos_of_rid[obs_perm[s]] = s;
}

// 6 x 6 (or narrower) blocks of Sigma the pass reads for the observations `pos` (sorted positions; null: all O):
// per landmark touched v^2 for its v valid incidences (twice for a landmark with more than 64 observations,
// whose t_f are formed once for Sigma_ll and again per batch of 64), per observation c^2 for its c blocks of A.
// *landmarks: the landmarks touched.
inline uint64_t lever_block_reads(int LM, uint32_t K, const std::vector<uint32_t>& lm_ptr,
                                  const std::vector<uint32_t>& obs_perm, const std::vector<uint32_t>& proj_pose,
                                  const std::vector<uint32_t>& proj_lm, const std::vector<uint32_t>& lm_ref_pose,
                                  const std::vector<int32_t>& pose_opt, const std::vector<int32_t>& lm_opt,
                                  const uint32_t* pos, uint32_t n, uint32_t* landmarks) {
  uint64_t reads = 0;
  std::vector<uint32_t> lms;
  auto sides = [&](uint32_t s) -> uint64_t {
    const uint32_t a = obs_perm[s], l = proj_lm[a];
    const bool listed = LM != 1 || proj_pose[a] != lm_ref_pose[l];
    uint64_t c = (listed && pose_opt[proj_pose[a]] >= 0) + (LM == 1 && listed && pose_opt[lm_ref_pose[l]] >= 0) + (K > 0);
    return c * c;
  };
  if (pos) {
    for (uint32_t q = 0; q < n; ++q) { reads += sides(pos[q]); lms.push_back(proj_lm[obs_perm[pos[q]]]); }
    std::sort(lms.begin(), lms.end());
    lms.erase(std::unique(lms.begin(), lms.end()), lms.end());
  } else {
    for (uint32_t s = 0; s < n; ++s) reads += sides(s);
    for (uint32_t l = 0; l + 1 < lm_ptr.size(); ++l)
      if (lm_ptr[l + 1] > lm_ptr[l]) lms.push_back(l);
  }
  for (uint32_t l : lms) {
    if (lm_opt[l] < 0) continue;
    const uint32_t nobs = lm_ptr[l + 1] - lm_ptr[l];
    uint64_t v = 0;
    bool any_listed = false;
    for (uint32_t s = lm_ptr[l]; s < lm_ptr[l + 1]; ++s) {
      const uint32_t pm = proj_pose[obs_perm[s]];
      if (LM == 1 && pm == lm_ref_pose[l]) continue;
      any_listed = true;
      v += pose_opt[pm] >= 0;
    }
    if (LM == 1 && any_listed && pose_opt[lm_ref_pose[l]] >= 0) ++v;
    if (K > 0) ++v;
    reads += v * v * (nobs > 64 ? 2 : 1);
  }
  if (landmarks) *landmarks = (uint32_t)lms.size();
  return reads;
}

// The device's inputs, on the host.  Observations are in sorted order (by landmark); Sigma is dense, n x n, in the
// engine's row order (pose_opt[p] * D .., then K calibration rows at np).
struct LeverHostIn {
  int LM = 1, D = 6, K = 0;
  uint32_t L = 0, O = 0, np = 0, n = 0, lrow_base = 0;
  const uint32_t *lm_ptr = nullptr, *obs_pose = nullptr, *lm_ref_pose = nullptr;
  const int32_t *pose_opt = nullptr, *lm_opt = nullptr;
  const double* frow = nullptr;     // factor rows (structure.h)
  const double* obs_jl = nullptr;   // [O][2 LM]
  const double* crow = nullptr;     // [2 O + L][6]: sqrt(w) dz_dk rows, then E_l; null without calibration
  const double* sigma = nullptr;
};

// variant 0: the formula.  Deliberately wrong ones, which the CPU suite must tell from it: 1 drops the sym2 cross
// term, 2 replaces Sigma_ll by V^-1, 3 drops the reference-pose block of A (LM == 1).
// out: [O][4] by sorted position, row-major 2 x 2, bitwise symmetric.
template <int LM>
inline void leverage_host_lm(const LeverHostIn& in, int variant, double* out) {
  const int R = LM == 1 ? 6 : 8, WO = LM == 1 ? 4 : 2;
  struct Ent { bool valid; uint32_t base; int width; const double* w; };
  auto sig = [&](uint32_t r, uint32_t c) { return in.sigma[(size_t)r * in.n + c]; };
  std::vector<Ent> ent;
  std::vector<double> t;
  for (uint32_t l = 0; l < in.L; ++l) {
    const uint32_t a0 = in.lm_ptr[l], nobs = in.lm_ptr[l + 1] - a0, rp = in.lm_ref_pose[l];
    if (!nobs) continue;
    const bool act = in.lm_opt[l] >= 0;
    bool any_listed = false;
    for (uint32_t e = 0; e < nobs; ++e) any_listed = any_listed || (LM == 1 && in.obs_pose[a0 + e] != rp);
    // the incidences, in lm_entry's order: observations, reference row (LM == 1), E_l (K > 0)
    ent.clear();
    for (uint32_t e = 0; e < nobs; ++e) {
      const uint32_t pm = in.obs_pose[a0 + e];
      const int po = in.pose_opt[pm];
      ent.push_back({!(LM == 1 && pm == rp) && po >= 0, po >= 0 ? (uint32_t)po * in.D : 0, 6,
                     in.frow + ((size_t)(a0 + e) * R + WO) * 6});
    }
    if (LM == 1) {
      const int po = in.pose_opt[rp];
      ent.push_back({any_listed && po >= 0, po >= 0 ? (uint32_t)po * in.D : 0, 6,
                     in.frow + ((size_t)in.lrow_base + 2 * (size_t)l) * 6});
    }
    if (in.K > 0) ent.push_back({in.crow != nullptr, in.np, in.K, in.crow ? in.crow + (2 * (size_t)in.O + l) * 6 : nullptr});
    const size_t ne = ent.size();
    // t_f[i][k] = sum_e sum_j Sigma[f + i][e + j] W_e[k][j]
    t.assign(ne * 6 * LM, 0.0);
    double U[LM][LM] = {{0}}, Li[LM][LM] = {{0}}, Q[LM][LM] = {{0}};
    if (act) {
      for (size_t f = 0; f < ne; ++f) {
        if (!ent[f].valid) continue;
        for (int i = 0; i < ent[f].width; ++i)
          for (size_t e = 0; e < ne; ++e) {
            if (!ent[e].valid) continue;
            for (int j = 0; j < ent[e].width; ++j) {
              const double sg = sig(ent[f].base + i, ent[e].base + j);
              for (int k = 0; k < LM; ++k) t[(f * 6 + i) * LM + k] += sg * ent[e].w[k * 6 + j];
            }
          }
        for (int k1 = 0; k1 < LM; ++k1)
          for (int k2 = 0; k2 < LM; ++k2)
            for (int i = 0; i < ent[f].width; ++i) U[k1][k2] += ent[f].w[k1 * 6 + i] * t[(f * 6 + i) * LM + k2];
      }
      double V[LM][LM] = {{0}};
      for (uint32_t e = 0; e < nobs; ++e) {
        const double* B = in.obs_jl + (size_t)(a0 + e) * 2 * LM;
        for (int a = 0; a < LM; ++a)
          for (int b = 0; b < LM; ++b) V[a][b] += B[a] * B[b] + B[LM + a] * B[LM + b];
      }
      lever_factor<LM>(V, Li);
      for (int a = 0; a < LM; ++a)
        for (int b = 0; b < LM; ++b) {
          double s = 0.0;
          for (int c = 0; c < LM; ++c)
            for (int d = 0; d < LM; ++d) s += Li[a][c] * U[c][d] * Li[b][d];
          Q[a][b] = (a == b ? 1.0 : 0.0) + (variant == 2 ? 0.0 : s);
        }
    }
    for (uint32_t e = 0; e < nobs; ++e) {
      const uint32_t a = a0 + e, pm = in.obs_pose[a];
      const bool listed = !(LM == 1 && pm == rp);
      // the blocks of A: measuring pose, reference pose, calibration
      struct Side { bool valid; uint32_t base; int width; const double* rows; size_t slot; } sd[3];
      sd[0] = {listed && in.pose_opt[pm] >= 0, in.pose_opt[pm] >= 0 ? (uint32_t)in.pose_opt[pm] * in.D : 0, 6,
               in.frow + (size_t)a * R * 6, e};
      sd[1] = {LM == 1 && listed && in.pose_opt[rp] >= 0 && variant != 3,
               in.pose_opt[rp] >= 0 ? (uint32_t)in.pose_opt[rp] * in.D : 0, 6, in.frow + ((size_t)a * R + 2) * 6, nobs};
      sd[2] = {in.K > 0 && in.crow, in.np, in.K, in.crow ? in.crow + 2 * (size_t)a * 6 : nullptr,
               (size_t)nobs + (LM == 1 ? 1 : 0)};
      double H[2][2] = {{0, 0}, {0, 0}};
      for (int f = 0; f < 3; ++f)
        for (int g = 0; g < 3; ++g) {
          if (!sd[f].valid || !sd[g].valid) continue;
          for (int r = 0; r < 2; ++r)
            for (int c = 0; c < 2; ++c)
              for (int i = 0; i < sd[f].width; ++i)
                for (int j = 0; j < sd[g].width; ++j)
                  H[r][c] += sd[f].rows[r * 6 + i] * sig(sd[f].base + i, sd[g].base + j) * sd[g].rows[c * 6 + j];
        }
      if (act) {
        const double* B = in.obs_jl + (size_t)a * 2 * LM;
        double At[2][LM] = {{0}};
        for (int f = 0; f < 3; ++f) {
          if (!sd[f].valid) continue;
          for (int r = 0; r < 2; ++r)
            for (int k = 0; k < LM; ++k)
              for (int i = 0; i < sd[f].width; ++i) At[r][k] += sd[f].rows[r * 6 + i] * t[(sd[f].slot * 6 + i) * LM + k];
        }
        double M[2][LM], N[2][LM], Z[2][LM];  // B Li^T, At Li^T, M Q
        for (int r = 0; r < 2; ++r)
          for (int k2 = 0; k2 < LM; ++k2) {
            double m = 0.0, nn = 0.0;
            for (int k = 0; k < LM; ++k) { m += B[r * LM + k] * Li[k2][k]; nn += At[r][k] * Li[k2][k]; }
            M[r][k2] = m; N[r][k2] = nn;
          }
        for (int r = 0; r < 2; ++r)
          for (int k2 = 0; k2 < LM; ++k2) {
            double z = 0.0;
            for (int k = 0; k < LM; ++k) z += M[r][k] * Q[k][k2];
            Z[r][k2] = z;
          }
        for (int r = 0; r < 2; ++r)
          for (int c = 0; c < 2; ++c) {
            double cr = 0.0, cc = 0.0, p = 0.0;
            for (int k = 0; k < LM; ++k) { cr += N[r][k] * M[c][k]; cc += N[c][k] * M[r][k]; p += Z[r][k] * M[c][k]; }
            H[r][c] += p - (variant == 1 ? 0.0 : cr + cc);
          }
      }
      const double h01 = 0.5 * (H[0][1] + H[1][0]);
      out[4 * (size_t)a] = H[0][0] + 0.0; out[4 * (size_t)a + 1] = h01 + 0.0;
      out[4 * (size_t)a + 2] = h01 + 0.0; out[4 * (size_t)a + 3] = H[1][1] + 0.0;
    }
  }
}

inline void leverage_host(const LeverHostIn& in, int variant, double* out) {
  if (in.LM == 1) leverage_host_lm<1>(in, variant, out);
  else leverage_host_lm<3>(in, variant, out);
}

}  // namespace bae
