// Joint covariance of an arbitrary set of parameters (ba_hip_get_joint_marginals) from the tile-sparse
// L D L^T that ba_hip_solve_gn leaves behind, without the selected inverse.  Plain C++17, no HIP: the
// launch code (k_jointcov.hip) and the CPU harness (hostcheck.cpp, tests/test_joint_marginals_plan.py)
// share the plan below, and jointcov_host restates the computation the kernels run.
//
// With S = L D L^T, D = diag(+-1), and the unit columns E of the m requested rows of S:
//   Sigma_sel,sel = E^T L^-T D L^-1 E = Y^T D Y,   Y = L^-1 E.
// Y is a forward substitution with m right-hand sides, by 64-row tiles
//   Y_I = L_II^-1 ( E_I - sum_{J < I, L_IJ != 0} L_IJ Y_J ),
// and Y_I is structurally zero unless tile row I lies on the elimination-tree path (parent = min R_J,
// R_J the rows below the diagonal of tile column J) from a requested tile to the root.  The union of
// those paths is the reach; only its tile rows are stored (one 64 x m_pad panel each) and visited, and
// only sources J inside it are read.  Every factor tile of the reach is used once per block of 64
// columns: sum_I |row(I) n reach| products in the substitution and |reach| in the epilogue.
#pragma once
#include <stdint.h>

#include "none_row.h"

#include <algorithm>
#include <vector>

namespace bae {

static const uint32_t kJointNone = kNoneRow;
static const uint32_t kJointChunk = 4;      // sources per chunk: the K loop of a row is split into
                                            // ceil(sources / 4) workgroups, their partial tiles summed in order
static const uint32_t kJointGramGroup = 8;  // reach rows per partial sum of the Gram product

struct JointPlan {
  uint32_t nt = 0;
  uint32_t m = 0;       // requested columns
  uint32_t ncb = 0;     // blocks of 64 columns
  uint32_t m_pad = 0;   // 64 ncb: leading dimension of a Y panel
  std::vector<uint32_t> reach;     // tile rows of the reach, ascending
  std::vector<uint32_t> pos;       // nt: position of a tile row in reach (its Y panel); kJointNone outside
  std::vector<uint32_t> level_of;  // per reach position: height above the rows without sources
  std::vector<uint32_t> src_ptr;   // reach + 1: sources of position q are src[src_ptr[q] .. src_ptr[q + 1]), tile rows, ascending
  std::vector<uint32_t> src;
  // Schedule.  Level v is one launch over its chunks (times ncb) and one over its rows (times ncb).
  // rows: 4 values per row in level order: tile row I, first chunk, end chunk (global chunk ids), first chunk
  // of the row's level (partial tile of chunk c and column block b: slot (c - first of level) ncb + b).
  // chunks: 4 values per chunk: tile row I, position of I, first source, end source (indices into src).
  std::vector<uint32_t> level_ptr;        // levels + 1, into rows / 4
  std::vector<uint32_t> rows;
  std::vector<uint32_t> chunk_level_ptr;  // levels + 1, into chunks / 4
  std::vector<uint32_t> chunks;
  uint32_t max_level_chunks = 0;          // slots needed: max_level_chunks ncb
  uint32_t gram_groups = 0;               // ceil(reach / kJointGramGroup)
  uint64_t products = 0;                  // ncb (sum_I |row(I) n reach| + |reach|)
  uint32_t levels() const { return level_ptr.empty() ? 0 : (uint32_t)level_ptr.size() - 1; }
  size_t y_count() const { return reach.size() * 64 * (size_t)m_pad; }
};

// nzL: nt x nt lower factor pattern (row-major bytes), tiles: the tile rows that hold a non-zero of any column of
// the right-hand side (for unit columns: the tile rows that hold a requested row; for the landmark columns of
// jointstate.h: the tile rows their incidences touch).  Repeats and any order are fine.
inline void build_joint_plan(const std::vector<uint8_t>& nzL, uint32_t nt, const std::vector<uint32_t>& tiles, uint32_t m,
                             JointPlan& p) {
  p = JointPlan();
  p.nt = nt;
  p.m = m;
  p.ncb = (m + 63) / 64;
  p.m_pad = 64 * p.ncb;
  std::vector<uint8_t> in(nt, 0);
  for (uint32_t t : tiles)
    for (uint32_t j = t; j < nt && !in[j];) {
      in[j] = 1;
      uint32_t par = nt;
      for (uint32_t i = j + 1; i < nt; ++i)
        if (nzL[(size_t)i * nt + j]) { par = i; break; }
      j = par;
    }
  p.pos.assign(nt, kJointNone);
  for (uint32_t j = 0; j < nt; ++j)
    if (in[j]) { p.pos[j] = (uint32_t)p.reach.size(); p.reach.push_back(j); }
  const uint32_t nr = (uint32_t)p.reach.size();
  p.src_ptr.assign((size_t)nr + 1, 0);
  p.level_of.assign(nr, 0);
  uint32_t depth = 0;
  for (uint32_t q = 0; q < nr; ++q) {
    const uint32_t I = p.reach[q];
    uint32_t lev = 0;
    for (uint32_t J = 0; J < I; ++J)
      if (in[J] && nzL[(size_t)I * nt + J]) {
        p.src.push_back(J);
        lev = std::max(lev, p.level_of[p.pos[J]] + 1);
      }
    p.src_ptr[q + 1] = (uint32_t)p.src.size();
    p.level_of[q] = lev;
    depth = std::max(depth, lev + 1);
  }
  if (nr == 0) depth = 0;
  p.level_ptr.assign((size_t)depth + 1, 0);
  p.chunk_level_ptr.assign((size_t)depth + 1, 0);
  for (uint32_t v = 0; v < depth; ++v) {
    const uint32_t cbase = (uint32_t)(p.chunks.size() / 4);
    for (uint32_t q = 0; q < nr; ++q) {
      if (p.level_of[q] != v) continue;
      const uint32_t I = p.reach[q], s0 = p.src_ptr[q], s1 = p.src_ptr[q + 1];
      const uint32_t c0 = (uint32_t)(p.chunks.size() / 4);
      for (uint32_t s = s0; s < s1; s += kJointChunk) {
        const uint32_t c[4] = {I, q, s, std::min(s + kJointChunk, s1)};
        p.chunks.insert(p.chunks.end(), c, c + 4);
      }
      const uint32_t r[4] = {I, c0, (uint32_t)(p.chunks.size() / 4), cbase};
      p.rows.insert(p.rows.end(), r, r + 4);
    }
    p.level_ptr[v + 1] = (uint32_t)(p.rows.size() / 4);
    p.chunk_level_ptr[v + 1] = (uint32_t)(p.chunks.size() / 4);
    p.max_level_chunks = std::max(p.max_level_chunks, p.chunk_level_ptr[v + 1] - cbase);
  }
  p.gram_groups = (nr + kJointGramGroup - 1) / kJointGramGroup;
  p.products = (uint64_t)p.ncb * ((uint64_t)p.src.size() + nr);
}

// One entry of a right-hand side column: B[row][col] += v (row: a row of S, col < m).
struct JointEntry {
  uint32_t row, col;
  double v;
};

// The substitution alone (k_joint_fsolve + k_joint_epilogue per level): the panels Y hold the right-hand side and
// take L^-1 of it.  Shared with the multi-RHS solve of factorsolve.h.
inline void joint_forward_host(const JointPlan& p, const double* L, size_t ld, const double* linvT, double* Y) {
  const uint32_t m = p.m, mp = p.m_pad;
  std::vector<double> part((size_t)64 * mp), T((size_t)64 * mp);
  for (uint32_t v = 0; v < p.levels(); ++v)
    for (uint32_t e = p.level_ptr[v]; e < p.level_ptr[v + 1]; ++e) {
      const uint32_t I = p.rows[4 * e], c0 = p.rows[4 * e + 1], c1 = p.rows[4 * e + 2];
      double* YI = Y + (size_t)p.pos[I] * 64 * mp;
      std::copy(YI, YI + (size_t)64 * mp, T.begin());
      for (uint32_t c = c0; c < c1; ++c) {
        std::fill(part.begin(), part.end(), 0.0);
        for (uint32_t s = p.chunks[4 * c + 2]; s < p.chunks[4 * c + 3]; ++s) {
          const uint32_t J = p.src[s];
          const double* LIJ = L + (size_t)I * 64 * ld + (size_t)J * 64;
          const double* YJ = Y + (size_t)p.pos[J] * 64 * mp;
          for (uint32_t r = 0; r < 64; ++r)
            for (uint32_t k = 0; k < 64; ++k) {
              const double l = LIJ[(size_t)r * ld + k];
              for (uint32_t x = 0; x < m; ++x) part[(size_t)r * mp + x] += l * YJ[(size_t)k * mp + x];
            }
        }
        for (size_t i = 0; i < part.size(); ++i) T[i] -= part[i];
      }
      const double* G = linvT + (size_t)I * 4096;  // G[c][x] = (L_II^-1)[x][c]
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t x = 0; x < m; ++x) {
          double s = 0.0;
          for (uint32_t k = 0; k < 64; ++k) s += G[k * 64 + r] * T[(size_t)k * mp + x];
          YI[(size_t)r * mp + x] = s;
        }
    }
}

// Host restatement of k_joint_init (+ k_joint_rhs), k_joint_fsolve + k_joint_epilogue per level, k_joint_gram and
// k_joint_combine, with the device's order of summation over chunks, slots and groups.  L: the factor in the
// engine's lower storage (row-major, leading dimension ld >= 64 nt; only tiles of the pattern are read),
// linvT: nt tiles L_JJ^-T (row-major), dsgn: 64 nt pivot signs.  The right-hand side B (64 nt x m) starts from
// zero and takes the `ne` entries in their order (entries that share a place add up); every entry's tile row must
// be one the plan was seeded with.  Y: reach x 64 x m_pad (the panels), cov = B^T S^-1 B: m x m row-major.
inline void jointcov_host_rhs(const JointPlan& p, const double* L, size_t ld, const double* linvT, const double* dsgn,
                              const JointEntry* ent, size_t ne, double* Y, double* cov) {
  const uint32_t m = p.m, mp = p.m_pad, nr = (uint32_t)p.reach.size();
  std::fill(Y, Y + p.y_count(), 0.0);
  for (size_t i = 0; i < ne; ++i) Y[((size_t)p.pos[ent[i].row / 64] * 64 + ent[i].row % 64) * mp + ent[i].col] += ent[i].v;
  joint_forward_host(p, L, ld, linvT, Y);
  std::vector<double> acc((size_t)m * m, 0.0), grp((size_t)m * m);
  for (uint32_t g = 0; g < p.gram_groups; ++g) {
    std::fill(grp.begin(), grp.end(), 0.0);
    for (uint32_t q = g * kJointGramGroup; q < std::min(nr, (g + 1) * kJointGramGroup); ++q) {
      const double* YI = Y + (size_t)q * 64 * mp;
      const double* d = dsgn + (size_t)p.reach[q] * 64;
      for (uint32_t k = 0; k < 64; ++k)
        for (uint32_t a = 0; a < m; ++a) {
          const double ya = YI[(size_t)k * mp + a] * d[k];
          for (uint32_t b = 0; b <= a; ++b) grp[(size_t)a * m + b] += ya * YI[(size_t)k * mp + b];
        }
    }
    for (size_t i = 0; i < acc.size(); ++i) acc[i] += grp[i];
  }
  for (uint32_t a = 0; a < m; ++a)
    for (uint32_t b = 0; b <= a; ++b) cov[(size_t)a * m + b] = cov[(size_t)b * m + a] = acc[(size_t)a * m + b];
}

// The unit-column case: sel, the m requested rows of S (column c is the unit vector of row sel[c]).
inline void jointcov_host(const JointPlan& p, const double* L, size_t ld, const double* linvT, const double* dsgn,
                          const uint32_t* sel, double* Y, double* cov) {
  std::vector<JointEntry> ent(p.m);
  for (uint32_t c = 0; c < p.m; ++c) ent[c] = {sel[c], c, 1.0};
  jointcov_host_rhs(p, L, ld, linvT, dsgn, ent.data(), ent.size(), Y, cov);
}

}  // namespace bae
