// Leverages of unary, binary and inertial residuals (ba_hip_get_pose_pose_leverages, k_pplever.hip): per residual
// the covariance of the predicted residual C = J Sigma_ee J^T, its effective information Lambda and the leverage
// tr(C Lambda), from what a direct solve leaves behind.  Plain C++17, no HIP: the block-read count serves the
// engine, and pose_pose_leverage_host restates the device formula over a dense Sigma for the CPU suite
// (hostcheck.cpp: ba_hostcheck_pose_pose_leverages, tests/test_pose_pose_leverages.py).
//
// Residual i couples the poses p1 and (binary, inertial) p2:
//   J      = [dz1 | dz2], R x 2 D, the UNWHITENED Jacobians of pp_dz; the column of a masked parameter and the
//            block of an inactive pose are zero (applied here, as k_pp_jrhs and k_pp_scatter apply them)
//   Lambda   the information for which J^T Lambda J is what the residual put into S:
//              unary     cov_inv * scale (the compounded Huber weights)              = pp_info
//              binary    weight * S^T S, S = cov_inv_sqrt as supplied (binary_blocks) - pp_info holds the
//                        UNWEIGHTED cov_inv there, which is not Lambda
//              inertial  cov_inv * Huber factor                                       = pp_info
//   Sigma_ee the block of Sigma = S^-1 over the rows of the live poses of the residual
//   C = J Sigma_ee J^T (symmetrised), leverage = tr(C Lambda).
// With Lambda = G G^T the whitened hat block is G^T C G; over all residual kinds of a system the traces sum to
// the number of unknowns.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define BAE_PPLEVER_FN __host__ __device__ __forceinline__
#else
#define BAE_PPLEVER_FN inline
#endif

namespace bae {

static const int kPPLevDim = 15;                       // storage width of every block: 15 x 15 row-major
static const int kPPLevBlock = kPPLevDim * kPPLevDim;
static const uint32_t kPPLevNoPose = 0xffffffffu;      // p2 of a unary residual

// element (r, c) of weight * S^T S for the 6 x 6 row-major S, zero outside 6 x 6
BAE_PPLEVER_FN double pplever_binary_info(const double* s36, double weight, int r, int c) {
  if (r >= 6 || c >= 6) return 0.0;
  double a = 0.0;
  for (int k = 0; k < 6; ++k) a += s36[k * 6 + r] * s36[k * 6 + c];
  return a * weight;
}

// D x D blocks of Sigma the pass stages for n residuals: (live poses)^2 each
inline uint64_t pplever_block_reads(uint32_t n, const uint32_t* p1, const uint32_t* p2, const int32_t* pose_opt) {
  uint64_t reads = 0;
  for (uint32_t q = 0; q < n; ++q) {
    const uint64_t live = (p1[q] != kPPLevNoPose && pose_opt[p1[q]] >= 0) + (p2[q] != kPPLevNoPose && pose_opt[p2[q]] >= 0);
    reads += live * live;
  }
  return reads;
}

// The device's inputs, on the host.  Sigma is dense, n x n, rows of pose p at pose_opt[p] * D.
struct PPLeverHostIn {
  int D = 6;
  uint32_t nres = 0, n = 0;
  const uint32_t *p1 = nullptr, *p2 = nullptr;   // [nres] pose ids; p2 = kPPLevNoPose for a unary residual
  const int32_t* pose_opt = nullptr;             // by pose id, negative: inactive
  const uint16_t* pose_mask = nullptr;           // by pose id, bit c: parameter c is masked
  const double* dz = nullptr;                    // [nres][2][225] dz1 | dz2, columns unmasked
  const double* info = nullptr;                  // [nres][225] information WITHOUT the weight
  const double* weight = nullptr;                // [nres], or null for 1: Lambda = weight * info
  const double* sigma = nullptr;
};

// variant 0: the formula.  Deliberately wrong ones, which the CPU suite must tell from it: 1 drops the cross block
// Sigma_{p1 p2}, 2 leaves the masked columns in J, 3 leaves the weight out of Lambda.
// cov, lam: [nres][225] (either may be null), lev: [nres] (may be null).
inline void pose_pose_leverage_host(const PPLeverHostIn& in, int variant, double* cov, double* lam, double* lev) {
  const int D = in.D, N = kPPLevDim;
  std::vector<double> sig, J, T, C(kPPLevBlock), L(kPPLevBlock);
  for (uint32_t q = 0; q < in.nres; ++q) {
    // the live sides, p1 first
    uint32_t base[2];
    int side[2], nl = 0;
    uint16_t mask[2];
    for (int s = 0; s < 2; ++s) {
      const uint32_t p = s == 0 ? in.p1[q] : in.p2[q];
      if (p == kPPLevNoPose || in.pose_opt[p] < 0) continue;
      base[nl] = (uint32_t)in.pose_opt[p] * (uint32_t)D;
      side[nl] = s;
      mask[nl] = variant == 2 ? 0 : in.pose_mask[p];
      ++nl;
    }
    const int m = nl * D;
    sig.assign((size_t)m * m, 0.0);
    J.assign((size_t)N * m, 0.0);
    T.assign((size_t)m * N, 0.0);
    for (int a = 0; a < nl; ++a)
      for (int b = 0; b < nl; ++b) {
        if (variant == 1 && a != b) continue;
        for (int i = 0; i < D; ++i)
          for (int j = 0; j < D; ++j)
            sig[(size_t)(a * D + i) * m + b * D + j] = in.sigma[(size_t)(base[a] + i) * in.n + base[b] + j];
      }
    for (int a = 0; a < nl; ++a)
      for (int r = 0; r < N; ++r)
        for (int c = 0; c < D; ++c)
          J[(size_t)r * m + a * D + c] =
              (mask[a] >> c) & 1 ? 0.0 : in.dz[((size_t)q * 2 + side[a]) * kPPLevBlock + r * N + c];
    for (int i = 0; i < m; ++i)
      for (int r = 0; r < N; ++r) {
        double s = 0.0;
        for (int j = 0; j < m; ++j) s += sig[(size_t)i * m + j] * J[(size_t)r * m + j];
        T[(size_t)i * N + r] = s;
      }
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < N; ++c) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s += J[(size_t)r * m + i] * T[(size_t)i * N + c];
        C[r * N + c] = s;
      }
    const double w = in.weight && variant != 3 ? in.weight[q] : 1.0;
    for (int k = 0; k < kPPLevBlock; ++k) L[k] = in.info[(size_t)q * kPPLevBlock + k] * w;
    double tr = 0.0;
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < N; ++c) {
        const double cs = 0.5 * (C[r * N + c] + C[c * N + r]) + 0.0;
        tr += cs * L[c * N + r];
        if (cov) cov[(size_t)q * kPPLevBlock + r * N + c] = cs;
      }
    if (lam)
      for (int k = 0; k < kPPLevBlock; ++k) lam[(size_t)q * kPPLevBlock + k] = L[k];
    if (lev) lev[q] = tr;
  }
}

}  // namespace bae
