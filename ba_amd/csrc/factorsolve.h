// Solves S X = B for a caller's block of right-hand sides (ba_hip_factor_solve) with the tile-sparse L D L^T
// that ba_hip_solve_gn leaves behind.  Plain C++17, no HIP: the launch code (k_factorsolve.hip) and the CPU
// harness (hostcheck.cpp, tests/test_factor_solve_plan.py) share the plan below, and factor_solve_host restates
// the computation the kernels run.
//
// With S = L D L^T, D = diag(+-1), by 64-row tiles:
//   forward    Y_I = L_II^-1 ( B_I - sum_{J < I, L_IJ != 0} L_IJ Y_J ),          I ascending
//   backward   X_J = L_JJ^-T ( D_J Y_J - sum_{I > J, L_IJ != 0} L_IJ^T X_I ),    J descending
// The solution is dense, so both passes visit every tile row: one 64 x m_pad panel per tile row, panel t at
// position t, and X overwrites Y in place (the sources of column J are finished rows I > J).
//
// The forward schedule is build_joint_plan (jointcov.h) seeded with every tile row.  The backward schedule is the
// same builder on the mirrored pattern R[a][b] = nzL[nt - 1 - b][nt - 1 - a], which is lower triangular again;
// its indices are mapped back afterwards, so the backward plan speaks of tile columns J and source rows I of
// nzL.  Level of J = 1 + max over its sources; the sources of a column are listed with I DESCENDING (ascending in
// the mirror), split into chunks of kJointChunk, and the partial tiles of a level sit in slots numbered inside it.
#pragma once
#include "jointcov.h"

#include <cmath>

namespace bae {

struct FactorSolvePlan {
  uint32_t nt = 0;
  JointPlan fwd;  // rows: (tile row I, chunks, ...), src: tile columns J < I ascending; pos is the identity
  JointPlan bwd;  // rows: (tile column J, chunks, ...), chunks: (J, J, sources), src: tile rows I > J descending.
                  // reach, pos, level_of and src_ptr stay in the mirror's numbering (position q = nt - 1 - J)
  uint64_t products() const { return fwd.products + bwd.products; }
  uint32_t max_level_chunks() const { return std::max(fwd.max_level_chunks, bwd.max_level_chunks); }
  uint32_t backward_level_of(uint32_t J) const { return bwd.level_of[nt - 1 - J]; }
};

inline void build_factor_solve_plan(const std::vector<uint8_t>& nzL, uint32_t nt, uint32_t m, FactorSolvePlan& p) {
  p = FactorSolvePlan();
  p.nt = nt;
  std::vector<uint32_t> all(nt);
  for (uint32_t t = 0; t < nt; ++t) all[t] = t;
  build_joint_plan(nzL, nt, all, m, p.fwd);
  std::vector<uint8_t> R((size_t)nt * nt, 0);
  for (uint32_t a = 0; a < nt; ++a)
    for (uint32_t b = 0; b <= a; ++b) R[(size_t)a * nt + b] = nzL[(size_t)(nt - 1 - b) * nt + (nt - 1 - a)];
  build_joint_plan(R, nt, all, m, p.bwd);
  for (size_t e = 0; e < p.bwd.rows.size(); e += 4) p.bwd.rows[e] = nt - 1 - p.bwd.rows[e];
  for (size_t c = 0; c < p.bwd.chunks.size(); c += 4) p.bwd.chunks[c] = p.bwd.chunks[c + 1] = nt - 1 - p.bwd.chunks[c];
  for (uint32_t& s : p.bwd.src) s = nt - 1 - s;
}

// Wrong on purpose, for the soundness checks of tests/test_factor_solve_plan.py (0 is the computation).
enum FactorSolveVariant {
  kFsolRight = 0,
  kFsolNoSigns = 1,        // D_J left out of the backward pass
  kFsolUntransposed = 2,   // L_IJ used where L_IJ^T belongs
  kFsolDropChunk = 3,      // the second chunk of every column left out
};

// Host restatement of k_joint_fsolve + k_joint_epilogue (forward) and k_fsol_bsolve + k_fsol_bepilogue (backward)
// per level, with the device's order of summation over chunks and slots.  L, linvT, dsgn: as for
// jointcov_host_rhs.  X: nt x 64 x m_pad panels, holding B in the factorised row order (zeros in padding rows
// and columns) on entry and S^-1 B on return.
inline void factor_solve_host(const FactorSolvePlan& fp, const double* L, size_t ld, const double* linvT, const double* dsgn,
                              double* X, int variant = kFsolRight) {
  joint_forward_host(fp.fwd, L, ld, linvT, X);
  const JointPlan& p = fp.bwd;
  const uint32_t m = p.m, mp = p.m_pad;
  std::vector<double> part((size_t)64 * mp), T((size_t)64 * mp);
  for (uint32_t v = 0; v < p.levels(); ++v)
    for (uint32_t e = p.level_ptr[v]; e < p.level_ptr[v + 1]; ++e) {
      const uint32_t J = p.rows[4 * e], c0 = p.rows[4 * e + 1], c1 = p.rows[4 * e + 2];
      double* XJ = X + (size_t)J * 64 * mp;
      for (uint32_t k = 0; k < 64; ++k)
        for (uint32_t x = 0; x < mp; ++x)
          T[(size_t)k * mp + x] = XJ[(size_t)k * mp + x] * (variant == kFsolNoSigns ? 1.0 : dsgn[(size_t)J * 64 + k]);
      for (uint32_t c = c0; c < c1; ++c) {
        if (variant == kFsolDropChunk && c == c0 + 1) continue;
        std::fill(part.begin(), part.end(), 0.0);
        for (uint32_t s = p.chunks[4 * c + 2]; s < p.chunks[4 * c + 3]; ++s) {
          const uint32_t I = p.src[s];
          const double* LIJ = L + (size_t)I * 64 * ld + (size_t)J * 64;
          const double* XI = X + (size_t)I * 64 * mp;
          for (uint32_t k = 0; k < 64; ++k)
            for (uint32_t r = 0; r < 64; ++r) {
              const double l = variant == kFsolUntransposed ? LIJ[(size_t)r * ld + k] : LIJ[(size_t)k * ld + r];
              for (uint32_t x = 0; x < m; ++x) part[(size_t)r * mp + x] += l * XI[(size_t)k * mp + x];
            }
        }
        for (size_t i = 0; i < part.size(); ++i) T[i] -= part[i];
      }
      const double* G = linvT + (size_t)J * 4096;  // G[r][k] = (L_JJ^-T)[r][k]
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t x = 0; x < m; ++x) {
          double s = 0.0;
          for (uint32_t k = 0; k < 64; ++k) s += G[r * 64 + k] * T[(size_t)k * mp + x];
          XJ[(size_t)r * mp + x] = s;
        }
    }
}

// ---- weakest modes: the eigenpairs of S of smallest magnitude (ba_hip_get_weakest_modes) -------------------
// Block inverse iteration with Rayleigh-Ritz on a block of p = min(64, n) vectors (one column block of the solve
// above); it needs S^-1 only, so it works after the in-place factorisation has destroyed S.  Per iteration:
//   1. Q from X by scaled SVQB, twice: G = X^T X, scaled by its diagonal, G_s = U Lambda U^T on the host,
//      directions with Lambda < p eps dropped (their columns become zero and stay zero), X <- X (D^-1/2 U Lambda^-1/2)
//   2. W = S^-1 Q
//   3. T = Q^T W symmetrised, T = V Theta V^T on the host, pairs ordered by descending |theta| (ties: by index)
//   4. W <- W V, Q <- Q V, R = W - Q Theta formed explicitly, column norms from the diagonal of R^T R
//   5. pair i has converged when |R_i| <= tolerance |theta_i|; stop when the k pairs of largest |theta| all have
//   6. otherwise X <- W V
// lambda_i = 1 / theta_i, mode i = column i of Q V.  The iteration below is shared, through `Ops`, by the device
// (k_factorsolve.hip: panels on the device, the 64 x 64 matrices on the host) and by weakest_modes_host.
//
// The start block is counter based: entry (row, column) of X_0 is splitmix64 of
//   seed * 0xD1342543DE82EF95 + 64 row + column
// mapped to [-1, 1) by its top 53 bits, `row` being the caller's row (so the start does not depend on the pose
// ordering).  Padding rows start at zero; the padding block of the factor is an identity decoupled from the rest,
// so they stay exactly zero (started non-zero they would converge to its artificial eigenvalue 1).
inline double mode_start_value(uint32_t seed, uint32_t row, uint32_t col) {
  uint64_t z = (uint64_t)seed * 0xD1342543DE82EF95ull + (uint64_t)row * 64 + col;
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 4503599627370496.0) - 1.0;
}

static const uint32_t kModeBlock = 64;     // columns of a panel of the iteration
static const uint32_t kModeMaxK = 32;      // pairs a caller may ask for
static const uint32_t kModeGramGroup = 8;  // tile rows per partial sum of the Gram products

// Eigen-decomposition of a symmetric n x n matrix (row-major, destroyed) by cyclic Jacobi: A = V diag(w) V^T,
// the columns of V (row-major n x n) orthonormal; the order of w is whatever the sweeps leave.
inline void jacobi_eigh(uint32_t n, double* A, double* V, double* w) {
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < n; ++j) V[(size_t)i * n + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    uint32_t rotations = 0;
    for (uint32_t p = 0; p + 1 < n; ++p)
      for (uint32_t q = p + 1; q < n; ++q) {
        const double apq = A[(size_t)p * n + q], app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
        if (apq == 0.0 || std::fabs(apq) <= 0.25 * 2.220446049250313e-16 * std::sqrt(std::fabs(app * aqq))) continue;
        ++rotations;
        const double th = (aqq - app) / (2.0 * apq);
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (uint32_t k = 0; k < n; ++k) {   // columns p, q
          const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
          A[(size_t)k * n + p] = c * akp - sn * akq;
          A[(size_t)k * n + q] = sn * akp + c * akq;
        }
        for (uint32_t k = 0; k < n; ++k) {   // rows p, q
          const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
          A[(size_t)p * n + k] = c * apk - sn * aqk;
          A[(size_t)q * n + k] = sn * apk + c * aqk;
        }
        A[(size_t)p * n + q] = A[(size_t)q * n + p] = 0.0;
        for (uint32_t k = 0; k < n; ++k) {
          const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
          V[(size_t)k * n + p] = c * vkp - sn * vkq;
          V[(size_t)k * n + q] = sn * vkp + c * vkq;
        }
      }
    if (!rotations) break;
  }
  for (uint32_t i = 0; i < n; ++i) w[i] = A[(size_t)i * n + i];
}

struct ModeOptions {
  double tolerance = 1e-8;
  uint32_t max_iterations = 50;
  uint32_t seed = 1;
};
struct ModeResult {
  uint32_t iterations = 0, converged = 0, block = 0;
  double residual_max = 0.0;
  double theta[kModeBlock] = {};   // Ritz values of S^-1, descending |theta|
  int panel = 0;                   // the panel that holds Q V
};

// Ops: three panels 0, 1, 2 of kModeBlock columns and
//   start(a, seed, p)          X_0 into panel a (columns >= p zero)
//   gram(a, b, G)              G (64 x 64 row-major, host) = X_a^T X_b
//   apply(a, M)                X_a <- X_a M (M 64 x 64 row-major, host)
//   copy(dst, src), solve(a)   X_a <- S^-1 X_a
//   residual(w, q, theta, r)   X_r = X_w - X_q diag(theta)
//   svqb_begin() / svqb_end(), solve_begin() / solve_end()   brackets for the caller's timing
template <class Ops>
inline void weakest_modes_iterate(Ops& ops, uint32_t n, uint32_t k, const ModeOptions& o, ModeResult& r) {
  const uint32_t B = kModeBlock, p = std::min(B, n);
  const double eps = 2.220446049250313e-16;
  std::vector<double> G((size_t)B * B), U((size_t)B * B), M((size_t)B * B), lam(B), d(B);
  int x = 0, w = 1;
  const int rr = 2;
  r = ModeResult();
  r.block = p;
  ops.start(x, o.seed, p);
  for (uint32_t it = 1; it <= std::max(o.max_iterations, 1u); ++it) {
    ops.svqb_begin();
    for (int rep = 0; rep < 2; ++rep) {
      ops.gram(x, x, G.data());
      for (uint32_t c = 0; c < B; ++c) d[c] = G[(size_t)c * B + c] > 0.0 ? 1.0 / std::sqrt(G[(size_t)c * B + c]) : 0.0;
      for (uint32_t i = 0; i < B; ++i)
        for (uint32_t j = 0; j <= i; ++j)
          M[(size_t)i * B + j] = M[(size_t)j * B + i] = d[i] * (0.5 * (G[(size_t)i * B + j] + G[(size_t)j * B + i])) * d[j];
      jacobi_eigh(B, M.data(), U.data(), lam.data());
      for (uint32_t i = 0; i < B; ++i)
        for (uint32_t j = 0; j < B; ++j)
          M[(size_t)i * B + j] = lam[j] >= p * eps ? d[i] * U[(size_t)i * B + j] / std::sqrt(lam[j]) : 0.0;
      ops.apply(x, M.data());
    }
    ops.svqb_end();
    ops.solve_begin();
    ops.copy(w, x);
    ops.solve(w);
    ops.solve_end();
    ops.gram(x, w, G.data());
    for (uint32_t i = 0; i < B; ++i)
      for (uint32_t j = 0; j <= i; ++j)
        M[(size_t)i * B + j] = M[(size_t)j * B + i] = 0.5 * (G[(size_t)i * B + j] + G[(size_t)j * B + i]);
    jacobi_eigh(B, M.data(), U.data(), lam.data());
    uint32_t idx[kModeBlock];
    for (uint32_t i = 0; i < B; ++i) idx[i] = i;
    std::stable_sort(idx, idx + B, [&](uint32_t a, uint32_t b) { return std::fabs(lam[a]) > std::fabs(lam[b]); });
    for (uint32_t j = 0; j < B; ++j) {
      r.theta[j] = lam[idx[j]];
      for (uint32_t i = 0; i < B; ++i) M[(size_t)i * B + j] = U[(size_t)i * B + idx[j]];
    }
    ops.apply(w, M.data());
    ops.apply(x, M.data());
    ops.residual(w, x, r.theta, rr);
    ops.gram(rr, rr, G.data());
    r.converged = 0;
    r.residual_max = 0.0;
    for (uint32_t i = 0; i < k; ++i) {
      const double nrm = std::sqrt(std::max(G[(size_t)i * B + i], 0.0)), th = std::fabs(r.theta[i]);
      const double rel = th > 0.0 ? nrm / th : INFINITY;
      if (rel <= o.tolerance) ++r.converged;
      r.residual_max = std::max(r.residual_max, rel);
    }
    r.iterations = it;
    r.panel = x;
    if (r.converged == k || it == std::max(o.max_iterations, 1u)) break;
    std::swap(x, w);   // X <- W V
  }
}

// Host restatement of ba_hip_get_weakest_modes on a factor as for factor_solve_host; rows of the panels are the
// factorised rows (n of them, then padding).  eigenvalues: k, modes: k x n row-major, unit 2-norm.
// pad_nonzero (wrong on purpose, for tests/test_weakest_modes.py): the padding rows start from the generator too.
struct HostModeOps {
  const FactorSolvePlan& plan;
  const double *L, *linvT, *dsgn;
  size_t ld;
  uint32_t n;
  bool pad_nonzero;
  std::vector<double> P[3];
  HostModeOps(const FactorSolvePlan& pl, const double* L_, size_t ld_, const double* linvT_, const double* dsgn_, uint32_t n_,
              bool pad)
      : plan(pl), L(L_), linvT(linvT_), dsgn(dsgn_), ld(ld_), n(n_), pad_nonzero(pad) {
    for (auto& v : P) v.assign((size_t)plan.nt * 64 * kModeBlock, 0.0);
  }
  void start(int a, uint32_t seed, uint32_t p) {
    const uint32_t rows = pad_nonzero ? plan.nt * 64 : n;
    for (uint32_t r = 0; r < rows; ++r)
      for (uint32_t c = 0; c < p; ++c) P[a][(size_t)r * kModeBlock + c] = mode_start_value(seed, r, c);
  }
  void gram(int a, int b, double* G) const {   // partial sums per group of tile rows, combined in order
    const uint32_t B = kModeBlock;
    std::fill(G, G + (size_t)B * B, 0.0);
    std::vector<double> grp((size_t)B * B);
    for (uint32_t t0 = 0; t0 < plan.nt; t0 += kModeGramGroup) {
      std::fill(grp.begin(), grp.end(), 0.0);
      for (uint32_t r = t0 * 64; r < std::min(plan.nt, t0 + kModeGramGroup) * 64; ++r)
        for (uint32_t i = 0; i < B; ++i) {
          const double xa = P[a][(size_t)r * B + i];
          if (xa == 0.0) continue;
          for (uint32_t j = 0; j < B; ++j) grp[(size_t)i * B + j] += xa * P[b][(size_t)r * B + j];
        }
      for (size_t e = 0; e < grp.size(); ++e) G[e] += grp[e];
    }
  }
  void apply(int a, const double* M) {
    const uint32_t B = kModeBlock;
    double row[kModeBlock];
    for (uint32_t r = 0; r < plan.nt * 64; ++r) {
      double* x = &P[a][(size_t)r * B];
      for (uint32_t j = 0; j < B; ++j) row[j] = 0.0;
      for (uint32_t k = 0; k < B; ++k)
        if (x[k] != 0.0)
          for (uint32_t j = 0; j < B; ++j) row[j] += x[k] * M[(size_t)k * B + j];
      std::copy(row, row + B, x);
    }
  }
  void copy(int dst, int src) { P[dst] = P[src]; }
  void solve(int a) { factor_solve_host(plan, L, ld, linvT, dsgn, P[a].data()); }
  void residual(int w, int q, const double* theta, int r) {
    for (size_t e = 0; e < P[r].size(); ++e) P[r][e] = P[w][e] - P[q][e] * theta[e % kModeBlock];
  }
  void svqb_begin() {}
  void svqb_end() {}
  void solve_begin() {}
  void solve_end() {}
};

// eigenvalues (k) and modes (k x n, unit 2-norm) out of the iteration's result; Qv: n x kModeBlock, rows in the
// caller's order
inline void modes_finish(const ModeResult& r, uint32_t n, uint32_t k, const double* Qv, double* eigenvalues, double* modes) {
  for (uint32_t i = 0; i < k; ++i) {
    eigenvalues[i] = 1.0 / r.theta[i];
    double s = 0.0;
    for (uint32_t row = 0; row < n; ++row) s += Qv[(size_t)row * kModeBlock + i] * Qv[(size_t)row * kModeBlock + i];
    const double inv = s > 0.0 ? 1.0 / std::sqrt(s) : 0.0;
    for (uint32_t row = 0; row < n; ++row) modes[(size_t)i * n + row] = Qv[(size_t)row * kModeBlock + i] * inv;
  }
}

inline void weakest_modes_host(const std::vector<uint8_t>& nzL, uint32_t nt, const double* L, size_t ld, const double* linvT,
                               const double* dsgn, uint32_t n, uint32_t k, const ModeOptions& o, bool pad_nonzero,
                               double* eigenvalues, double* modes, ModeResult& r) {
  FactorSolvePlan plan;
  build_factor_solve_plan(nzL, nt, kModeBlock, plan);
  HostModeOps ops(plan, L, ld, linvT, dsgn, n, pad_nonzero);
  weakest_modes_iterate(ops, n, k, o, r);
  modes_finish(r, n, k, ops.P[r.panel].data(), eigenvalues, modes);
}

}  // namespace bae
