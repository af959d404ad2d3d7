// Selected inverse of the reduced camera system (ba_hip_compute_marginals): the blocks of
// Sigma = S^-1 on the tile pattern of the factor L, from the tile-sparse L D L^T that
// ba_hip_solve_gn leaves behind.  Plain C++17, no HIP: the launch code (k_selinv.hip) and the CPU
// harness (hostcheck.cpp, tests/test_selected_inverse.py) share the column schedule and the slot
// index below, and selinv_host restates the recursion the kernels run.
//
// Recursion.  L carries sqrt|pivot| and D = diag(+-1), so S = L D L^T and Sigma = L^-T D L^-1.
// From Sigma L = L^-T D, walking the 64x64 tile columns J from the last to the first with
// R_J = { K > J : L_KJ structurally nonzero }:
//   Sigma_IJ = -( sum_{K in R_J} Sigma_IK L_KJ ) L_JJ^-1                       I in R_J
//   Sigma_JJ = L_JJ^-T D_J L_JJ^-1 - ( sum_{K in R_J} Sigma_KJ^T L_KJ ) L_JJ^-1
// with Sigma_IK = Sigma_KI^T when I < K.  R_J is a clique of the closed symbolic fill
// (tile_symbolic_factor), so every Sigma_IK the recursion reads lies in L's pattern, and the
// recursion produces exactly the tiles of that pattern: the compact store holds one 64x64 slot
// (row-major) per lower tile of nzL, diagonal tiles in full.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace bae {

static const uint32_t kNoSlot = 0xffffffffu;

struct SelinvPlan {
  uint32_t nt = 0;
  uint32_t n_slots = 0;
  std::vector<uint32_t> slot;      // nt x nt: slot of lower tile (i, k), i >= k; kNoSlot outside the pattern
  std::vector<uint32_t> col_ptr;   // nt + 1: R_J of column J is col_rows[col_ptr[J] .. col_ptr[J + 1]), ascending
  std::vector<uint32_t> col_rows;
  uint64_t products = 0;           // 64x64x64 tile products: sum_J |R_J|^2 (column tiles) + nt (diagonal tiles)
  uint32_t max_rows = 0;           // max_J |R_J|
  // Schedule.  Column J reads the Sigma tiles of the columns in R_J, all of them ancestors of J in the
  // elimination tree (parent = min R_J).  Columns of one tree level are therefore independent: level
  // v (0 = the roots) is one launch of k_selinv_col over all its (J, I in R_J) items and one launch of
  // k_selinv_diag over its columns, levels from the roots down.  A banded (natural order) pattern is a
  // chain, one column per level; an ordering with a bushy tree runs many columns per launch.
  std::vector<uint32_t> level_ptr;   // levels + 1: columns of level v are level_cols[level_ptr[v] .. level_ptr[v + 1])
  std::vector<uint32_t> level_cols;
  std::vector<uint32_t> item_ptr;    // levels + 1: items of level v are items[2 item_ptr[v] .. 2 item_ptr[v + 1]) as (J, I)
  std::vector<uint32_t> items;
};

// Tile products of the selected inverse on a lower factor pattern (nt x nt bytes, row-major).
inline uint64_t selinv_tile_products(const std::vector<uint8_t>& nzL, uint32_t nt) {
  uint64_t total = nt;
  for (uint64_t j = 0; j < nt; ++j) {
    uint64_t m = 0;
    for (uint64_t i = j + 1; i < nt; ++i) m += nzL[i * nt + j] ? 1 : 0;
    total += m * m;
  }
  return total;
}

inline void build_selinv_plan(const std::vector<uint8_t>& nzL, uint32_t nt, SelinvPlan& p) {
  p.nt = nt;
  p.slot.assign((size_t)nt * nt, kNoSlot);
  p.col_ptr.assign((size_t)nt + 1, 0);
  p.col_rows.clear();
  p.max_rows = 0;
  uint32_t s = 0;
  for (uint32_t i = 0; i < nt; ++i)
    for (uint32_t k = 0; k <= i; ++k)
      if (k == i || nzL[(size_t)i * nt + k]) p.slot[(size_t)i * nt + k] = s++;
  p.n_slots = s;
  for (uint32_t j = 0; j < nt; ++j) {
    for (uint32_t i = j + 1; i < nt; ++i)
      if (nzL[(size_t)i * nt + j]) p.col_rows.push_back(i);
    p.col_ptr[j + 1] = (uint32_t)p.col_rows.size();
    p.max_rows = std::max(p.max_rows, p.col_ptr[j + 1] - p.col_ptr[j]);
  }
  p.products = selinv_tile_products(nzL, nt);
  std::vector<uint32_t> level(nt, 0);
  uint32_t depth = 0;
  for (uint32_t j = nt; j-- > 0;) {
    level[j] = p.col_ptr[j + 1] > p.col_ptr[j] ? level[p.col_rows[p.col_ptr[j]]] + 1 : 0;
    depth = std::max(depth, level[j] + 1);
  }
  p.level_ptr.assign((size_t)depth + 1, 0);
  for (uint32_t j = 0; j < nt; ++j) p.level_ptr[level[j] + 1]++;
  for (uint32_t v = 0; v < depth; ++v) p.level_ptr[v + 1] += p.level_ptr[v];
  p.level_cols.assign(nt, 0);
  {
    std::vector<uint32_t> cur(p.level_ptr.begin(), p.level_ptr.end() - 1);
    for (uint32_t j = 0; j < nt; ++j) p.level_cols[cur[level[j]]++] = j;
  }
  p.item_ptr.assign((size_t)depth + 1, 0);
  p.items.clear();
  for (uint32_t v = 0; v < depth; ++v) {
    for (uint32_t q = p.level_ptr[v]; q < p.level_ptr[v + 1]; ++q) {
      const uint32_t j = p.level_cols[q];
      for (uint32_t e = p.col_ptr[j]; e < p.col_ptr[j + 1]; ++e) { p.items.push_back(j); p.items.push_back(p.col_rows[e]); }
    }
    p.item_ptr[v + 1] = (uint32_t)(p.items.size() / 2);
  }
}

// Element (r, c) of Sigma from the compact store (both halves: the upper one by symmetry);
// NaN outside the pattern.
inline double selinv_element(const SelinvPlan& p, const double* store, uint32_t r, uint32_t c) {
  uint32_t tr = r / 64, tc = c / 64;
  if (tr < tc) { const uint32_t t = r; r = c; c = t; tr = r / 64; tc = c / 64; }
  const uint32_t s = p.slot[(size_t)tr * p.nt + tc];
  if (s == kNoSlot) return __builtin_nan("");
  return store[(size_t)s * 4096 + (size_t)(r % 64) * 64 + (c % 64)];
}

// Host restatement of the device recursion (k_selinv_col, then k_selinv_diag, per column; the columns
// from the last, which is one of the orders the level schedule allows).  L: the factor in the engine's lower storage (row-major, leading dimension ld >= 64 nt; only
// the tiles of the pattern are read), linvT: nt tiles L_JJ^-T (row-major), dsgn: 64 nt pivot signs.
// store: n_slots x 4096 doubles.
inline void selinv_host(const SelinvPlan& p, const double* L, size_t ld, const double* linvT, const double* dsgn,
                        double* store) {
  const uint32_t nt = p.nt;
  std::vector<double> T(4096), M(4096);
  auto tile = [&](uint32_t i, uint32_t k) { return store + (size_t)p.slot[(size_t)i * nt + k] * 4096; };
  // Sigma_IK (row r, column x), either half
  auto sig = [&](uint32_t I, uint32_t K, uint32_t r, uint32_t x) {
    return I >= K ? tile(I, K)[r * 64 + x] : tile(K, I)[x * 64 + r];
  };
  for (uint32_t J = nt; J-- > 0;) {
    const uint32_t* R = p.col_rows.data() + p.col_ptr[J];
    const uint32_t m = p.col_ptr[J + 1] - p.col_ptr[J];
    const double* G = linvT + (size_t)J * 4096;  // G[c][x] = (L_JJ^-1)[x][c]
    for (uint32_t a = 0; a < m; ++a) {
      const uint32_t I = R[a];
      std::fill(T.begin(), T.end(), 0.0);
      for (uint32_t b = 0; b < m; ++b) {
        const uint32_t K = R[b];
        const double* LKJ = L + (size_t)K * 64 * ld + (size_t)J * 64;
        for (uint32_t r = 0; r < 64; ++r)
          for (uint32_t x = 0; x < 64; ++x) {
            const double s = sig(I, K, r, x);
            for (uint32_t c = 0; c < 64; ++c) T[r * 64 + c] += s * LKJ[(size_t)x * ld + c];
          }
      }
      double* out = tile(I, J);
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t c = 0; c < 64; ++c) {
          double s = 0.0;
          for (uint32_t x = 0; x < 64; ++x) s += T[r * 64 + x] * G[c * 64 + x];
          out[r * 64 + c] = -s;
        }
    }
    std::fill(T.begin(), T.end(), 0.0);
    for (uint32_t b = 0; b < m; ++b) {
      const uint32_t K = R[b];
      const double* LKJ = L + (size_t)K * 64 * ld + (size_t)J * 64;
      const double* SKJ = tile(K, J);
      for (uint32_t x = 0; x < 64; ++x)
        for (uint32_t r = 0; r < 64; ++r) {
          const double s = SKJ[x * 64 + r];
          for (uint32_t c = 0; c < 64; ++c) T[r * 64 + c] += s * LKJ[(size_t)x * ld + c];
        }
    }
    for (uint32_t r = 0; r < 64; ++r)
      for (uint32_t x = 0; x < 64; ++x) M[r * 64 + x] = G[r * 64 + x] * dsgn[(size_t)J * 64 + x] - T[r * 64 + x];
    double* out = tile(J, J);
    for (uint32_t r = 0; r < 64; ++r)
      for (uint32_t c = 0; c < 64; ++c) {
        double s = 0.0;
        for (uint32_t x = 0; x < 64; ++x) s += M[r * 64 + x] * G[c * 64 + x];
        out[r * 64 + c] = s;
      }
  }
}

}  // namespace bae
