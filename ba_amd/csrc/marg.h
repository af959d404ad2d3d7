// Sliding-window marginalisation (ba_hip_marginalize) and the dense pose prior residual
// (ba_hip_set_dense_priors).  Plain C++17 plus the prior's error-state map, which k_marg.hip and the
// CPU test harness (hostcheck.cpp, tests/test_marginalization_plan.py) share.
//
// ---- the prior's error state -----------------------------------------------------------------------
// d(x) is the delta ApplyUpdate needs to take x0 to x (x = x0 [+] (-d), k_apply_poses):
//     d_t = t0 - t,   d_w = log(q^-1 q0),   d_v = v0 - v,   d_b = b0 - b.
// J_d = dd(x [+] (-delta)) / ddelta at delta = 0 is the identity except for the rotation block, the
// inverse left Jacobian of SO(3) at d_w (log(exp(delta) exp(d_w)) = d_w + Jl^-1(d_w) delta + ..).
//
// ---- the plan of one marginalisation ----------------------------------------------------------------
// marg_plan classifies the residuals of the host Problem, builds the local
// index map [M | B] (M in the caller's order, the blanket B sorted by pose id) and, per D x D block
// (I >= J) of the local system and per local pose, a fixed-order list of terms that k_marg_assemble sums:
//   block terms (MargTerm.kind)
//     0  projection rank-1 term: element (r, c) += frow[a][r] * frow[b][c]   (r, c < 6)
//     1  pose-pose slot a, part b: 0 H11, 1 H12, 2 H12^T, 3 H22 of pp_h
//     2  dense prior a: rows of its pose b, columns of its pose c of the linearised J^T H J
//   rhs terms
//     0  frow[a][r] * scal[b];   1  pp_g of slot a, side b;   2  prior a, pose b of J^T (b - H d)
//   error terms
//     0  scal of observation a, squared;   1  -b_l^T V_l^-1 b_l of landmark a;   2  pp error of slot a;
//     3  E_p of prior a
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dpose.h"
#include "structure.h"

namespace bae {

// ---- error state of a dense prior (host and device) ---------------------------------------------------
// Jl^-1(w) = I - 1/2 [w]x + (1/th^2 - (1 + cos th) / (2 th sin th)) [w]x^2
BA_HD void so3_left_jacobian_inv(const double* w, double* J9) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double th = sqrt(th2);
  const double f = th < 1e-5 ? 1.0 / 12.0 + th2 / 720.0 : 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
  const double A[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double a2 = 0.0;
      for (int k = 0; k < 3; ++k) a2 += A[r * 3 + k] * A[k * 3 + c];
      J9[r * 3 + c] = (r == c ? 1.0 : 0.0) - 0.5 * A[r * 3 + c] + f * a2;
    }
}

// x0, x: 16-double pose states t(3) q(4) v(3) b(6); d: D doubles; J: D x D row-major or null
BA_HD void prior_delta(const double* x0, const double* x, int D, double* d, double* J) {
  for (int i = 0; i < 3; ++i) d[i] = x0[i] - x[i];
  const double qc[4] = {-x[3], -x[4], -x[5], x[6]};
  double r[4];
  bad::quat_mul(qc, x0 + 3, r);
  bad::quat_normalize(r);
  const bad::V3 w = bad::so3_log(r);
  d[3] = w.x; d[4] = w.y; d[5] = w.z;
  for (int i = 6; i < D; ++i) d[i] = x0[i + 1] - x[i + 1];
  if (!J) return;
  for (int i = 0; i < D * D; ++i) J[i] = 0.0;
  for (int i = 0; i < D; ++i) J[i * D + i] = 1.0;
  double R[9];
  so3_left_jacobian_inv(d + 3, R);
  for (int r2 = 0; r2 < 3; ++r2)
    for (int c = 0; c < 3; ++c) J[(3 + r2) * D + 3 + c] = R[r2 * 3 + c];
}

// ---- limits ---------------------------------------------------------------------------------------------
static const uint32_t kMargMaxM = 128;     // |M| * D: S^a_MM is factorised by one workgroup
static const uint32_t kMargMaxB = 4096;    // |B| * D: H is (|B| D)^2 doubles (128 MiB)

// The dense priors of a problem: CSR over their poses (ids of the problem), per prior x0 (16 per pose),
// H (k D x k D row-major), b (k D), c.
struct DensePriors {
  std::vector<uint32_t> ptr{0}, pose;
  std::vector<double> x0, H, b, c;
  std::vector<size_t> h_off;  // first H entry of every prior (ptr-derived)
  uint32_t count() const { return (uint32_t)ptr.size() - 1; }
  void offsets(int D) {
    h_off.assign(count() + 1, 0);
    for (uint32_t q = 0; q < count(); ++q) {
      const size_t k = (size_t)(ptr[q + 1] - ptr[q]) * D;
      h_off[q + 1] = h_off[q] + k * k;
    }
  }
};

struct MargTerm { uint32_t kind, a, b, c; };  // same layout as HIP's uint4

struct MargPlan {
  uint32_t nM = 0, nB = 0;                     // local poses: [0, nM) = M, [nM, nM + nB) = B
  std::vector<uint32_t> local_pose;            // pose id of every local pose
  std::vector<uint32_t> blk_ij;                // per lower block: I << 16 | J
  std::vector<uint32_t> blk_ptr;               // CSR over blk_ij into blk_terms
  std::vector<MargTerm> blk_terms;
  std::vector<uint32_t> rhs_ptr;               // per local pose
  std::vector<MargTerm> rhs_terms;
  std::vector<MargTerm> err_terms;
  // counts of ba_hip_marginalization_stats
  uint32_t n_proj = 0, n_unary = 0, n_binary = 0, n_imu = 0, n_prior = 0, n_dropped = 0;
};

// Returns false and sets err on a refused request.  pose_opt: the engine's optimisation ids (< 0: inactive);
// lm_ptr / obs_perm: observations sorted by landmark (structure.h); R, lrow_base: factor-row layout.
inline bool marg_plan(const Problem& pb, int LM, int D, const std::vector<int32_t>& pose_opt,
                      const std::vector<uint32_t>& lm_ptr, const std::vector<uint32_t>& obs_perm, uint32_t R,
                      uint32_t lrow_base, const DensePriors& pr, const uint32_t* m_ids, uint32_t nm,
                      const uint32_t* l_ids, uint32_t nl, MargPlan& pl, std::string& err) {
  pl = MargPlan();
  const uint32_t P = pb.num_poses, L = pb.num_lms, O = pb.num_proj;
  const uint32_t NONE = 0xffffffffu;
  if (nm == 0) { err = "marginalize: the pose set M is empty"; return false; }
  std::vector<uint32_t> loc(P, NONE);
  for (uint32_t i = 0; i < nm; ++i) {
    const uint32_t p = m_ids[i];
    if (p >= P) { err = "marginalize: pose " + std::to_string(p) + " does not exist"; return false; }
    if (pose_opt[p] < 0) { err = "marginalize: pose " + std::to_string(p) + " is inactive"; return false; }
    if (loc[p] != NONE) { err = "marginalize: pose " + std::to_string(p) + " is listed twice"; return false; }
    loc[p] = i;
  }
  if ((uint64_t)nm * D > kMargMaxM) {
    err = "marginalize: |M| * PoseSize exceeds " + std::to_string(kMargMaxM);
    return false;
  }
  if (nl && LM == 0) { err = "marginalize: landmarks given with LmSize 0"; return false; }
  std::vector<uint8_t> inL(L, 0);
  for (uint32_t i = 0; i < nl; ++i) {
    const uint32_t l = l_ids[i];
    if (l >= L) { err = "marginalize: landmark " + std::to_string(l) + " does not exist"; return false; }
    if (!pb.lm_active[l]) { err = "marginalize: landmark " + std::to_string(l) + " is inactive"; return false; }
    if (inL[l]) { err = "marginalize: landmark " + std::to_string(l) + " is listed twice"; return false; }
    inL[l] = 1;
  }
  auto inM = [&](uint32_t p) { return p < P && loc[p] != NONE && loc[p] < nm; };
  if (LM == 1)
    for (uint32_t l = 0; l < L; ++l)
      if (pb.lm_active[l] && !inL[l] && inM(pb.lm_ref_pose[l])) {
        err = "marginalize: landmark " + std::to_string(l) + " is anchored in a marginalised pose but not in L";
        return false;
      }
  // ---- blanket: active poses outside M that appear in an absorbed residual, by pose id
  std::vector<uint8_t> inB(P, 0);
  auto touch = [&](uint32_t p) { if (p < P && pose_opt[p] >= 0 && !inM(p)) inB[p] = 1; };
  auto listed = [&](uint32_t a) { return LM != 1 || pb.proj_pose[a] != pb.lm_ref_pose[pb.proj_lm[a]]; };
  for (uint32_t a = 0; a < O; ++a) {
    const uint32_t l = pb.proj_lm[a];
    if (!pb.lm_active[l]) continue;
    if (inL[l]) {
      if (!listed(a)) continue;
      touch(pb.proj_pose[a]);
      if (LM == 1) touch(pb.lm_ref_pose[l]);
    } else if (inM(pb.proj_pose[a])) {
      pl.n_dropped++;
    }
  }
  for (uint32_t i = 0; i < nl; ++i)
    for (uint32_t s = lm_ptr[l_ids[i]]; s < lm_ptr[l_ids[i] + 1]; ++s) pl.n_proj++;
  const uint32_t nu = pb.num_unary, nb = pb.num_binary, ni = pb.num_imu;
  std::vector<uint32_t> abs_slot;  // absorbed pose-pose slots [unary | binary | imu], in slot order
  for (uint32_t i = 0; i < nu; ++i)
    if (inM(pb.un_pose[i])) { abs_slot.push_back(i); pl.n_unary++; }
  for (uint32_t i = 0; i < nb; ++i)
    if (inM(pb.bin_p1[i]) || inM(pb.bin_p2[i])) {
      abs_slot.push_back(nu + i); pl.n_binary++;
      touch(pb.bin_p1[i]); touch(pb.bin_p2[i]);
    }
  for (uint32_t i = 0; i < ni; ++i)
    if (inM(pb.imu_p1[i]) || inM(pb.imu_p2[i])) {
      abs_slot.push_back(nu + nb + i); pl.n_imu++;
      touch(pb.imu_p1[i]); touch(pb.imu_p2[i]);
    }
  std::vector<uint32_t> abs_prior;
  for (uint32_t q = 0; q < pr.count(); ++q) {
    bool any = false;
    for (uint32_t k = pr.ptr[q]; k < pr.ptr[q + 1]; ++k) any = any || inM(pr.pose[k]);
    if (!any) continue;
    abs_prior.push_back(q); pl.n_prior++;
    for (uint32_t k = pr.ptr[q]; k < pr.ptr[q + 1]; ++k) touch(pr.pose[k]);
  }
  pl.nM = nm;
  pl.local_pose.assign(m_ids, m_ids + nm);
  for (uint32_t p = 0; p < P; ++p)
    if (inB[p]) { loc[p] = nm + pl.nB++; pl.local_pose.push_back(p); }
  if ((uint64_t)pl.nB * D > kMargMaxB) {
    err = "marginalize: the blanket has " + std::to_string(pl.nB) + " poses, |B| * PoseSize exceeds " +
          std::to_string(kMargMaxB);
    return false;
  }
  const uint32_t n = pl.nM + pl.nB;
  auto lp = [&](uint32_t p) -> uint32_t { return (p < P && pose_opt[p] >= 0) ? loc[p] : NONE; };
  // ---- terms: per lower block (I >= J) in a flat n x n table first, then compacted to CSR
  std::vector<std::vector<MargTerm>> blk((size_t)n * (n + 1) / 2), rhs(n);
  auto bidx = [](uint32_t I, uint32_t J) { return (size_t)I * (I + 1) / 2 + J; };
  auto add2 = [&](uint32_t I, uint32_t J, MargTerm t) { blk[bidx(I, J)].push_back(t); };  // I >= J
  const uint32_t WO = (uint32_t)w_row_offset(LM);
  struct Inc { uint32_t I, wrow; };
  std::vector<Inc> inc;
  for (uint32_t i = 0; i < nl; ++i) {
    const uint32_t l = l_ids[i];
    // J^T J of every observation: its measuring side (u, v rows at s R) and reference side (s R + 2)
    inc.clear();
    bool any = false;
    for (uint32_t s = lm_ptr[l]; s < lm_ptr[l + 1]; ++s) {
      const uint32_t a = obs_perm[s];
      pl.err_terms.push_back({0, s, 0, 0});
      if (!listed(a)) continue;
      any = true;
      const uint32_t m = lp(pb.proj_pose[a]);
      const uint32_t r = LM == 1 ? lp(pb.lm_ref_pose[l]) : NONE;
      for (uint32_t k = 0; k < 2; ++k) {
        if (m != NONE) {
          add2(m, m, {0, s * R + k, s * R + k, 0});
          rhs[m].push_back({0, s * R + k, 2 * s + k, 0});
        }
        if (r != NONE) {
          add2(r, r, {0, s * R + 2 + k, s * R + 2 + k, 0});
          rhs[r].push_back({0, s * R + 2 + k, 2 * s + k, 0});
        }
        if (m != NONE && r != NONE && m != r) {
          if (m > r) add2(m, r, {0, s * R + k, s * R + 2 + k, 0});
          else add2(r, m, {0, s * R + 2 + k, s * R + k, 0});
        }
      }
      if (m != NONE) inc.push_back({m, s * R + WO});
    }
    if (LM == 1 && any && lp(pb.lm_ref_pose[l]) != NONE) inc.push_back({lp(pb.lm_ref_pose[l]), lrow_base + 2 * l});
    // -W V^-1 W^T: every ordered pair of incidences, element (r, c) += W_x[r] (-W_y V^-1)[c]
    for (const Inc& x : inc) {
      for (const Inc& y : inc) {
        if (x.I < y.I) continue;
        for (int k = 0; k < LM; ++k) add2(x.I, y.I, {0, x.wrow + k, y.wrow + LM + k, 0});
      }
      for (int k = 0; k < LM; ++k) rhs[x.I].push_back({0, x.wrow + LM + k, 2 * O + l * LM + k, 0});
    }
    pl.err_terms.push_back({1, l, 0, 0});
  }
  for (uint32_t slot : abs_slot) {
    uint32_t p1, p2 = NONE;
    if (slot < nu) p1 = pb.un_pose[slot];
    else if (slot < nu + nb) { p1 = pb.bin_p1[slot - nu]; p2 = pb.bin_p2[slot - nu]; }
    else { p1 = pb.imu_p1[slot - nu - nb]; p2 = pb.imu_p2[slot - nu - nb]; }
    if (p2 == p1) p2 = NONE;  // (k_pp_scatter: a residual on one pose twice adds H11 and g1 only)
    const uint32_t I1 = lp(p1), I2 = p2 == NONE ? NONE : lp(p2);
    if (I1 != NONE) { add2(I1, I1, {1, slot, 0, 0}); rhs[I1].push_back({1, slot, 0, 0}); }
    if (I2 != NONE) { add2(I2, I2, {1, slot, 3, 0}); rhs[I2].push_back({1, slot, 1, 0}); }
    if (I1 != NONE && I2 != NONE) {
      if (I1 > I2) add2(I1, I2, {1, slot, 1, 0});
      else add2(I2, I1, {1, slot, 2, 0});
    }
    pl.err_terms.push_back({2, slot, 0, 0});
  }
  for (uint32_t q : abs_prior) {
    const uint32_t k0 = pr.ptr[q], k = pr.ptr[q + 1] - k0;
    for (uint32_t i = 0; i < k; ++i) {
      const uint32_t I = lp(pr.pose[k0 + i]);
      if (I == NONE) continue;
      rhs[I].push_back({2, q, i, 0});
      for (uint32_t j = 0; j < k; ++j) {
        const uint32_t J = lp(pr.pose[k0 + j]);
        if (J == NONE || J > I) continue;
        add2(I, J, {2, q, i, j});
      }
    }
    pl.err_terms.push_back({3, q, 0, 0});
  }
  for (uint32_t I = 0; I < n; ++I)
    for (uint32_t J = 0; J <= I; ++J) {
      const std::vector<MargTerm>& v = blk[bidx(I, J)];
      if (v.empty() && I != J) continue;
      if (pl.blk_ptr.empty()) pl.blk_ptr.push_back(0);
      pl.blk_ij.push_back(I << 16 | J);
      pl.blk_terms.insert(pl.blk_terms.end(), v.begin(), v.end());
      pl.blk_ptr.push_back((uint32_t)pl.blk_terms.size());
    }
  pl.rhs_ptr.assign(1, 0);
  for (uint32_t I = 0; I < n; ++I) {
    pl.rhs_terms.insert(pl.rhs_terms.end(), rhs[I].begin(), rhs[I].end());
    pl.rhs_ptr.push_back((uint32_t)pl.rhs_terms.size());
  }
  return true;
}

}  // namespace bae
