// Panel PCG (ba_hip_pcg_panel_solve_system, ba_hip_get_joint_marginals_pcg): X = S^-1 B for m <= 512 right-hand
// sides after a PCG solve, when A still holds S and there is no factor.  It is the solver of pcg.h run per column:
// m INDEPENDENT conjugate-gradient recurrences in lock-step, not block CG.  Every column has its own PcgState and
// its own pcg_decide (alpha, beta, true-residual verification, residual replacement, breakdown code, iteration
// count); only the tiles of S are shared: one pass reads them once per block of 64 columns and multiplies them with
// the panel on the FP64 matrix cores (k_pcg_panel.hip).  Plain C++17, no HIP: the launch code and the CPU harness
// (hostcheck.cpp, tests/test_pcg_panel_plan.py) share the plan and the shape of every sum; pcg_panel_host restates
// the passes.  Preconditioner: block-Jacobi only (the blocks of pcg_row_blocks, inverted once per call).
//
// Panels are (64 nt) x m_pad row-major, m_pad = 64 ceil(m / 64); padding columns are zero right-hand sides.
//
// Product Q = S P, per tile row I and block of 64 columns.  The sources of tile row I, in this order:
//   the tiles (I, J), J < I ascending     A_IJ P_J        (A_IJ is the index-major operand of tile_mma.h)
//   the diagonal tile                      A_II P_I        (symmetrised while it is staged: element (i, k), k > i, is
//                                                           read at (k, i); the upper triangle in memory is never read)
//   the tiles (I', I), I' > I ascending    A_I'I^T P_I'    (A_I'I as it lies is the k-major operand)
// They are cut into chunks of kPcgPanelChunk sources; one workgroup forms the partial tile of one (chunk, column
// block) in the slot of that pair, summing its sources in order, k ascending; the epilogue sums the slots of a
// tile row in chunk order.  No atomics, no memory-side adds: the bits do not depend on the launch order.
//
// Per-column sums (p.q, r.z, r.r) of the 64 rows of a tile row: four partial sums over the rows rs, rs + 4, ..,
// rs + 60 (rs = 0 .. 3, ascending), then (s0 + s2) + (s1 + s3); the tile rows are added in ascending order.  The
// sum of column j involves the values of column j only and does not depend on where in the panel the column sits.
//
// One pass: [spmm -> epilogue -> alpha] (not in pass 0) -> update1 -> decide -> update2.  A column whose state is
// `done` is frozen: its x, r and p are no longer written.  A column on its way to the verification holds x in its p
// from then on (a failed verification restarts with p = z, the old direction is dead): the product always reads P.
#pragma once
#include "pcg.h"

namespace bae {

static const uint32_t kPcgPanelMaxColumns = 512;   // BA_HIP_PCG_PANEL_MAX_COLUMNS
static const uint32_t kPcgPanelChunk = 8;          // sources per partial tile (slot traffic)
enum : uint32_t { kPanelRow = 0, kPanelDiag = 1, kPanelCol = 2 };
static const uint32_t kPcgPanelToX = 8;            // action bit beside kPcgStep / kPcgDir / kPcgRestart: p = x

struct PcgPanelPlan {
  uint32_t nt = 0, m = 0, m_pad = 0, ncb = 0;
  std::vector<uint32_t> src;        // 2 per source: (the other tile index: J, I or I'; kind)
  std::vector<uint32_t> chunks;     // 4 per chunk: (I, first source, end source, 0); slot = chunk index
  std::vector<uint32_t> chunk_ptr;  // nt + 1: the chunks of tile row I
  uint32_t n_src() const { return (uint32_t)(src.size() / 2); }
  uint32_t n_chunks() const { return (uint32_t)(chunks.size() / 4); }
  // per pass: 64 x 64 x 64 products, bytes read (tiles, panel tiles, slots back, P in the epilogue)
  double products() const { return (double)n_src() * ncb; }
  double bytes_read() const { return 32768.0 * ncb * (2.0 * n_src() + n_chunks() + nt); }
  size_t slot_doubles() const { return (size_t)n_chunks() * ncb * 4096; }
};

inline void build_pcg_panel_plan(const PcgPlan& pl, uint32_t m, PcgPanelPlan& p) {
  const uint32_t nt = pl.nt;
  p.nt = nt; p.m = m; p.m_pad = 64 * ((m + 63) / 64); p.ncb = p.m_pad / 64;
  p.src.clear(); p.chunks.clear();
  p.chunk_ptr.assign((size_t)nt + 1, 0);
  for (uint32_t I = 0; I < nt; ++I) {
    const uint32_t first = p.n_src();
    for (uint32_t s = pl.row_ptr[I]; s < pl.row_ptr[I + 1]; ++s) {   // ascending J, the diagonal tile last
      const uint32_t J = pl.tiles[2 * s + 1];
      p.src.push_back(J); p.src.push_back(J == I ? kPanelDiag : kPanelRow);
    }
    for (uint32_t e = pl.col_ptr[I]; e < pl.col_ptr[I + 1]; ++e) {   // ascending row, without the diagonal tile
      const uint32_t R = pl.tiles[2 * pl.col_slot[e]];
      if (R != I) { p.src.push_back(R); p.src.push_back(kPanelCol); }
    }
    const uint32_t end = p.n_src();
    for (uint32_t c = first; c < end; c += kPcgPanelChunk) {
      p.chunks.push_back(I); p.chunks.push_back(c); p.chunks.push_back(std::min(end, c + kPcgPanelChunk)); p.chunks.push_back(0);
    }
    p.chunk_ptr[I + 1] = p.n_chunks();
  }
}

// sum over the 64 rows of a tile row in the shape of the kernels (see above); v: stride `ld` between rows
inline double pcg_panel_colsum(const double* v, size_t ld = 1) {
  double s[4];
  for (uint32_t rs = 0; rs < 4; ++rs) {
    s[rs] = 0.0;
    for (uint32_t q = 0; q < 16; ++q) s[rs] += v[(size_t)(rs + 4 * q) * ld];
  }
  return (s[0] + s[2]) + (s[1] + s[3]);
}

// Deliberately wrong variants for the tests of the tests (tests/test_pcg_panel_plan.py): never used by the engine.
enum : int { kPanelRight = 0, kPanelWrongFrozenUpdated = 1, kPanelWrongDiagUpper = 2, kPanelWrongSharedAlpha = 3 };

// Q = S P as k_pcgp_spmm + k_pcgp_spmm_epilogue form it, and the per-tile-row partials of p.q.  A: lower storage,
// leading dimension ld = 64 nt; P, Q: ld x m (the restatement keeps the m real columns only: the padding columns are
// zero columns and no column reads another).  skip[j] != 0: column j is not formed (frozen).
inline void pcg_panel_spmm_host(const PcgPanelPlan& pp, const double* A, size_t ld, const double* P, uint32_t m,
                                const uint8_t* skip, double* Q, double* pq_part, int variant = kPanelRight) {
  std::vector<double> a(4096), part((size_t)64 * m), q((size_t)64 * m);   // a[k][i]; part, q: [j][i]
  for (uint32_t I = 0; I < pp.nt; ++I) {
    std::fill(q.begin(), q.end(), 0.0);
    for (uint32_t c = pp.chunk_ptr[I]; c < pp.chunk_ptr[I + 1]; ++c) {
      std::fill(part.begin(), part.end(), 0.0);
      for (uint32_t s = pp.chunks[4 * c + 1]; s < pp.chunks[4 * c + 2]; ++s) {
        const uint32_t T = pp.src[2 * s], kind = pp.src[2 * s + 1];
        for (uint32_t k = 0; k < 64; ++k)
          for (uint32_t i = 0; i < 64; ++i) {
            double v;
            if (kind == kPanelRow) v = A[(size_t)(I * 64 + i) * ld + (size_t)T * 64 + k];
            else if (kind == kPanelCol) v = A[(size_t)(T * 64 + k) * ld + (size_t)I * 64 + i];
            else if (variant == kPanelWrongDiagUpper) v = A[(size_t)(I * 64 + i) * ld + (size_t)I * 64 + k];
            else v = A[(size_t)(I * 64 + std::max(i, k)) * ld + (size_t)I * 64 + std::min(i, k)];
            a[k * 64 + i] = v;
          }
        for (uint32_t j = 0; j < m; ++j) {
          if (skip && skip[j]) continue;
          double* pj = &part[(size_t)j * 64];
          for (uint32_t k = 0; k < 64; ++k) {   // k ascending, as the matrix cores take their groups of four
            const double pk = P[(size_t)(T * 64 + k) * m + j];
            for (uint32_t i = 0; i < 64; ++i) pj[i] += a[k * 64 + i] * pk;
          }
        }
      }
      for (size_t e = 0; e < q.size(); ++e) q[e] += part[e];   // the epilogue: slots in chunk order
    }
    for (uint32_t j = 0; j < m; ++j) {
      if (skip && skip[j]) continue;
      double v[64];
      for (uint32_t i = 0; i < 64; ++i) {
        const size_t off = (size_t)(I * 64 + i) * m + j;
        Q[off] = q[(size_t)j * 64 + i];
        v[i] = P[off] * Q[off];
      }
      if (pq_part) pq_part[(size_t)I * m + j] = pcg_panel_colsum(v);
    }
  }
}

struct PcgPanelResult {
  uint32_t passes = 0;
  std::vector<PcgResult> col;   // per column (passes unused)
};

// The solver, pass by pass as the device runs it.  B, X: ld x m row-major (rows n .. ld are padding: identity rows
// of A, zero right-hand sides).  Returns 0, or 4 (BA_HIP_FACTORIZATION_ERROR) when some column broke down.
inline int pcg_panel_host(const PcgPlan& pl, const PcgPanelPlan& pp, const double* A, size_t ld, const double* B, uint32_t m,
                          uint32_t n, const std::vector<uint8_t>& nz, const std::vector<uint32_t>& blk,
                          const std::vector<uint32_t>& blocks, double rel_tolerance, uint32_t max_it, double* X,
                          PcgPanelResult* res, int variant = kPanelRight) {
  const uint32_t nt = pl.nt;
  const size_t N = ld * (size_t)m;
  std::vector<double> minv, R[2], Z(N, 0.0), P(N, 0.0), Q(N, 0.0);
  R[0].assign(N, 0.0);
  R[1].assign(N, 0.0);
  const int block_status = pcg_blocks_host(A, ld, nz, nt, blocks, minv);
  std::fill(X, X + N, 0.0);
  std::vector<PcgState> st[2];
  PcgState s0 = {};
  s0.tol2 = rel_tolerance * rel_tolerance;
  s0.max_it = max_it ? max_it : n;
  s0.mode = kPcgInit;
  st[0].assign(m, s0);
  st[1].assign(m, s0);
  std::vector<double> pq_part((size_t)nt * m, 0.0), rz_part((size_t)nt * m, 0.0), rr_part((size_t)nt * m, 0.0);
  std::vector<double> pq(m, 0.0), alpha1(m, 0.0), last_alpha(m, 0.0), last_beta(m, 0.0);
  std::vector<uint8_t> run(m, 0), frozen(m, 0);
  std::vector<uint32_t> last_act(m, 0);
  uint32_t k = 0;
  for (; k < pcg_max_passes(s0.max_it); ++k) {
    const std::vector<PcgState>& cur = st[k & 1];
    std::vector<PcgState>& nxt = st[(k + 1) & 1];
    bool all = true;
    for (uint32_t j = 0; j < m; ++j) { frozen[j] = cur[j].done ? 1 : 0; all = all && cur[j].done; }
    if (all) break;
    const std::vector<double>& rin = R[k & 1];
    std::vector<double>& rout = R[(k + 1) & 1];
    if (k > 0) pcg_panel_spmm_host(pp, A, ld, P.data(), m, frozen.data(), Q.data(), pq_part.data(), variant);
    for (uint32_t j = 0; j < m; ++j) {   // k_pcgp_alpha
      const PcgState& s = cur[j];
      double sum = 0.0, a = 0.0;
      bool go = !s.done;
      if (!s.done && s.mode == kPcgIter) {
        for (uint32_t I = 0; I < nt; ++I) sum += pq_part[(size_t)I * m + j];
        a = s.rz_old / sum;
        go = pcg_finite(sum) && sum > 0.0 && pcg_finite(a);
      }
      pq[j] = sum; alpha1[j] = a; run[j] = go ? 1 : 0;
    }
    if (variant == kPanelWrongSharedAlpha)
      for (uint32_t j = 1; j < m; ++j)
        if (run[j] && cur[j].mode == kPcgIter && !cur[0].done && cur[0].mode == kPcgIter) alpha1[j] = alpha1[0];
    for (uint32_t I = 0; I < nt; ++I)   // k_pcgp_update1
      for (uint32_t j = 0; j < m; ++j) {
        if (!run[j]) continue;
        const uint32_t mode = cur[j].mode;
        double vz[64], vr[64];
        for (uint32_t i = 0; i < 64; ++i) {
          const size_t row = (size_t)I * 64 + i;
          double rn = 0.0, zz = 0.0;
          if (row < n) {
            const uint32_t start = blk[2 * row], D = blk[2 * row + 1];
            for (uint32_t t = 0; t < D; ++t) {
              const size_t off = (size_t)(start + t) * m + j;
              const double rj = mode == kPcgIter ? rin[off] - alpha1[j] * Q[off] : mode == kPcgInit ? B[off] : B[off] - Q[off];
              if (start + t == row) rn = rj;
              zz += minv[row * 16 + t] * rj;
            }
          }
          rout[row * m + j] = rn;
          Z[row * m + j] = zz;
          vz[i] = rn * zz;
          vr[i] = rn * rn;
        }
        rz_part[(size_t)I * m + j] = pcg_panel_colsum(vz);
        rr_part[(size_t)I * m + j] = pcg_panel_colsum(vr);
      }
    for (uint32_t j = 0; j < m; ++j) {   // k_pcgp_decide, k_pcgp_update2
      const PcgState& s = cur[j];
      nxt[j] = s;
      uint32_t act = 0;
      double alpha = 0.0, beta = 0.0;
      if (!s.done) {
        double rz = 0.0, rr = 0.0;
        if (run[j])
          for (uint32_t I = 0; I < nt; ++I) { rz += rz_part[(size_t)I * m + j]; rr += rr_part[(size_t)I * m + j]; }
        act = pcg_decide(s, pq[j], rz, rr, block_status, nxt[j], alpha, beta);
        if (variant == kPanelWrongSharedAlpha && (act & kPcgStep) && !cur[0].done && cur[0].mode == kPcgIter) alpha = alpha1[0];
        if (!nxt[j].done && nxt[j].mode == kPcgVerify) act |= kPcgPanelToX;
        if (act & kPcgStep) { last_act[j] = act; last_alpha[j] = alpha; last_beta[j] = beta; }
      } else if (variant == kPanelWrongFrozenUpdated) {   // the column's last step, again
        act = last_act[j]; alpha = last_alpha[j]; beta = last_beta[j];
      }
      if (!act) continue;
      for (size_t row = 0; row < ld; ++row) {
        const size_t off = row * m + j;
        const double pv = P[off];
        double xv = X[off];
        if (act & kPcgStep) { xv += alpha * pv; X[off] = xv; }
        if (act & kPcgDir) P[off] = Z[off] + beta * pv;
        else if (act & kPcgRestart) P[off] = Z[off];
        if (act & kPcgPanelToX) P[off] = xv;
      }
    }
  }
  const std::vector<PcgState>& f = st[k & 1];
  bool broke = false;
  if (res) { res->passes = k; res->col.assign(m, PcgResult()); }
  for (uint32_t j = 0; j < m; ++j) {
    broke = broke || f[j].breakdown;
    if (!res) continue;
    PcgResult& r = res->col[j];
    r.iterations = f[j].iterations; r.converged = f[j].converged; r.replacements = f[j].replacements;
    r.breakdown = f[j].breakdown; r.passes = k; r.rr_recur = f[j].rr_recur; r.rr_true = f[j].rr_true; r.bb = f[j].bb;
  }
  return broke ? 4 : 0;
}

}  // namespace bae
