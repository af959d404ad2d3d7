// Iterative solve of the reduced camera system (ba_hip_set_reduced_solver, BA_HIP_SOLVER_PCG): conjugate
// gradients on S, preconditioned by its diagonal blocks (one D x D block per active pose, one K x K block for
// the calibration unknowns) — the inexact Gauss-Newton of Agarwal et al., "Bundle adjustment in the large".
// Plain C++17, no HIP: the launch code (k_pcg.hip) and the CPU harness (hostcheck.cpp, tests/test_pcg_plan.py)
// share the plan, the block inversion, the decision logic of one iteration and the shape of every reduction
// below; pcg_host restates the whole solver the kernels run.
//
// Operator.  q = S v over the lower tiles of S's OWN pattern (nzS, before fill).  Tile (I, J), I >= J, is read
// once and gives two 64-vectors: its row sums A_IJ v_J (slot `row`) and its column sums A_IJ^T v_I (slot `col`);
// of a diagonal tile only the lower triangle is read: the row sums take it with the diagonal, the column sums
// take the strict part.  q_I is then the sum of the row slots of tile row I in ascending J followed by the column
// slots of tile column I in ascending row — no atomics, the bits do not depend on the launch order.
//
// One pass of the solver is: [operator on p (or on x, to verify)] -> update1 -> update2.  update1 forms
// r, z = M^-1 r and the partial sums of r.z and r.r; update2 sums them, decides (pcg_decide) and moves x and p.
// The state lives on the device in two copies: pass k reads copy k & 1 and writes the other, so that no block
// reads a word another block of the same launch writes.  r is double buffered in the same way (z = M^-1 r reads
// the neighbours' rows of r).  Once `done` is set every further launch is a no-op.
//
// Two-level preconditioner (ba_hip_pcg_options.coarse_aggregate = g > 0, k_pcg_coarse.hip): M^-1 = M_bj^-1 +
// Z (Z^T S Z)^-1 Z^T, Z summing parameter d of the g consecutive poses of an aggregate (natural order) into one
// coarse unknown; the K calibration unknowns are coarse unknowns of their own.  C = Z^T S Z is assembled entry by
// entry, every entry as ONE sum over the fine rows and columns of its two coarse unknowns in natural order: the
// bits of C do not depend on where a pose ordering puts the rows (per-tile partial sums would).  C^-1 is formed
// explicitly (blocked Cholesky on 64-tiles, triangular inverse, L^-T L^-1, symmetrised); a pass then runs
// update1 -> restriction r_c = Z^T r -> y_c = C^-1 r_c -> update2 with z = z_bj + Z y_c and r.z = r.z_bj + r_c.y_c.
#pragma once
#include <stdint.h>

#include "none_row.h"

#include <algorithm>
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define PCG_HD __host__ __device__
#else
#define PCG_HD
#endif

namespace bae {

static const uint32_t kPcgMaxBlock = 16;   // largest preconditioner block (PoseSize 15)
static const uint32_t kPcgCoarseMax = 1024;   // BA_HIP_PCG_COARSE_MAX: coarse unknowns
static const uint32_t kPcgNone = kNoneRow;
enum : uint32_t { kPcgInit = 0, kPcgIter = 1, kPcgVerify = 2 };
enum : uint32_t { kPcgStep = 1 /* x += alpha p */, kPcgDir = 2 /* p = z + beta p */, kPcgRestart = 4 /* p = z */ };

struct PcgState {
  double rz_old, bb, rr_recur, rr_true, tol2;
  uint32_t mode, done, iterations, converged, replacements, breakdown, max_it, pad;
};

struct PcgPlan {
  uint32_t nt = 0, n_tiles = 0;
  std::vector<uint32_t> tiles;     // 2 n_tiles: (I, J) of slot s, ordered by I, then J
  std::vector<uint32_t> row_ptr;   // nt + 1: the slots of tile row I are row_ptr[I] .. row_ptr[I + 1]
  std::vector<uint32_t> col_ptr;   // nt + 1: the slots of tile column J are col_slot[col_ptr[J] .. col_ptr[J + 1]),
  std::vector<uint32_t> col_slot;  //         ascending row, the diagonal tile first
  double bytes_per_spmv = 0.0;     // tiles read + slots written and read back + the vectors
  // two-level preconditioner (build_pcg_coarse; coarse_req = 0: none)
  uint32_t coarse_req = 0, coarse_g = 0;   // aggregate size asked for / used (raised until nc <= kPcgCoarseMax)
  uint32_t nc = 0, ncp = 0, naggr = 0;     // coarse unknowns, padded to 64, aggregates
  std::vector<uint32_t> cmap;       // ld: coarse unknown of matrix row r, kPcgNone for padding rows
  std::vector<uint32_t> crow_ptr;   // nc + 1: the fine rows of coarse unknown c are crow_rows[crow_ptr[c] .. crow_ptr[c + 1]),
  std::vector<uint32_t> crow_rows;  //         in ascending natural order (ascending rows without a pose ordering)
};

// nz: nt x nt bytes, lower part read; diagonal tiles always belong to the operator.
inline void build_pcg_plan(const std::vector<uint8_t>& nz, uint32_t nt, PcgPlan& p) {
  p.nt = nt;
  p.tiles.clear();
  p.row_ptr.assign((size_t)nt + 1, 0);
  p.col_ptr.assign((size_t)nt + 1, 0);
  for (uint32_t i = 0; i < nt; ++i) {
    for (uint32_t j = 0; j <= i; ++j)
      if (j == i || nz[(size_t)i * nt + j]) { p.tiles.push_back(i); p.tiles.push_back(j); p.col_ptr[j + 1]++; }
    p.row_ptr[i + 1] = (uint32_t)(p.tiles.size() / 2);
  }
  p.n_tiles = (uint32_t)(p.tiles.size() / 2);
  for (uint32_t j = 0; j < nt; ++j) p.col_ptr[j + 1] += p.col_ptr[j];
  p.col_slot.assign(p.n_tiles, 0);
  std::vector<uint32_t> cur(p.col_ptr.begin(), p.col_ptr.end() - 1);
  for (uint32_t s = 0; s < p.n_tiles; ++s) p.col_slot[cur[p.tiles[2 * s + 1]]++] = s;
  p.bytes_per_spmv = (double)p.n_tiles * (32768.0 + 2.0 * 1024.0) + 3.0 * 512.0 * nt;
}

// (start, size) of the preconditioner block of every row, 2 uint32 per row of the padded system: np rows in
// blocks of D (the last one shorter if D does not divide np), then one block of K; size 0 = padding (M = 1).
inline void pcg_row_blocks(uint32_t np, uint32_t D, uint32_t K, uint32_t ld, std::vector<uint32_t>& blk,
                           std::vector<uint32_t>& blocks) {
  blk.assign((size_t)2 * ld, 0);
  blocks.clear();
  for (uint32_t s = 0; s < np; s += D) { blocks.push_back(s); blocks.push_back(std::min(D, np - s)); }
  if (K) { blocks.push_back(np); blocks.push_back(K); }
  for (size_t b = 0; b < blocks.size(); b += 2)
    for (uint32_t r = 0; r < blocks[b + 1]; ++r) { blk[2 * (size_t)(blocks[b] + r)] = blocks[b]; blk[2 * (size_t)(blocks[b] + r) + 1] = blocks[b + 1]; }
}

// nat_of_row: ld entries, the natural index of the unknown in matrix row r (nblk blocks of D unknowns, block-major,
// then K border unknowns; a short last block simply lacks its trailing unknowns) or kPcgNone for padding rows.
// Coarse unknown of natural index i < nblk D: (i / D / g) D + i % D; border unknown k: naggr D + k.  A coarse
// unknown without fine rows (only a short last block in its aggregate) is kept, with C = 1 on its diagonal.
inline void build_pcg_coarse(PcgPlan& p, const std::vector<uint32_t>& nat_of_row, uint32_t nblk, uint32_t D, uint32_t K,
                             uint32_t g_req) {
  uint32_t g = std::min(std::max(g_req, 1u), std::max(nblk, 1u));   // one aggregate for everything is the largest
  while ((uint64_t)D * ((nblk + g - 1) / g) + K > kPcgCoarseMax && g < nblk) ++g;
  p.coarse_req = g_req;
  p.coarse_g = g;
  p.naggr = (nblk + g - 1) / g;
  p.nc = D * p.naggr + K;
  p.ncp = std::max(((p.nc + 63) / 64) * 64, 64u);
  const uint32_t ld = (uint32_t)nat_of_row.size(), nn = nblk * D + K;
  std::vector<uint32_t> row_of_nat(nn, kPcgNone);
  for (uint32_t r = 0; r < ld; ++r)
    if (nat_of_row[r] != kPcgNone) row_of_nat[nat_of_row[r]] = r;
  auto coarse = [&](uint32_t i) { return i < nblk * D ? (i / D / g) * D + i % D : p.naggr * D + (i - nblk * D); };
  p.cmap.assign(ld, kPcgNone);
  p.crow_ptr.assign((size_t)p.nc + 1, 0);
  for (uint32_t i = 0; i < nn; ++i)
    if (row_of_nat[i] != kPcgNone) { p.cmap[row_of_nat[i]] = coarse(i); p.crow_ptr[coarse(i) + 1]++; }
  for (uint32_t c = 0; c < p.nc; ++c) p.crow_ptr[c + 1] += p.crow_ptr[c];
  p.crow_rows.assign(p.crow_ptr[p.nc], 0);
  std::vector<uint32_t> cur(p.crow_ptr.begin(), p.crow_ptr.end() - 1);
  for (uint32_t i = 0; i < nn; ++i)
    if (row_of_nat[i] != kPcgNone) p.crow_rows[cur[coarse(i)]++] = row_of_nat[i];
}

// nat_of_row of a system whose rows are in natural order: np rows in blocks of D, then K border rows
inline void pcg_natural_rows(uint32_t np, uint32_t D, uint32_t K, uint32_t ld, std::vector<uint32_t>& nat_of_row, uint32_t& nblk) {
  nblk = (np + D - 1) / D;
  nat_of_row.assign(ld, kPcgNone);
  for (uint32_t r = 0; r < np; ++r) nat_of_row[r] = r;
  for (uint32_t k = 0; k < K; ++k) nat_of_row[np + k] = nblk * D + k;
}

// In-place Gauss-Jordan inversion of a symmetric D x D block (a: 16 x 16 row-major), without pivoting: the
// pivots are those of L D L^T, so "every pivot > 0" is the test for positive definiteness.  Column j is what
// lane j of k_pcg_blocks owns.  Returns false on a pivot that is not positive and finite.
inline bool pcg_invert_block(double* a, uint32_t D) {
  bool ok = true;
  for (uint32_t k = 0; k < D; ++k) {
    const double p = a[k * 16 + k];
    const bool good = p > 0.0 && std::isfinite(p);
    if (!good) ok = false;
    const double ip = good ? 1.0 / p : 0.0;
    double f[16], rk[16];
    for (uint32_t i = 0; i < D; ++i) f[i] = a[i * 16 + k];
    for (uint32_t j = 0; j < D; ++j) rk[j] = j == k ? ip : a[k * 16 + j] * ip;
    for (uint32_t j = 0; j < D; ++j) {
      for (uint32_t i = 0; i < D; ++i)
        if (i != k) a[i * 16 + j] = j == k ? -f[i] * ip : a[i * 16 + j] - f[i] * rk[j];
      a[k * 16 + j] = rk[j];
    }
  }
  return ok;
}

// sum of 2^m values in the shape of the kernels' LDS trees (w = n / 2 .. 1: v[t] += v[t + w])
inline double pcg_tree(double* v, uint32_t n) {
  for (uint32_t w = n / 2; w > 0; w >>= 1)
    for (uint32_t t = 0; t < w; ++t) v[t] += v[t + w];
  return v[0];
}
// sum of n partials as one block of 256 threads forms it: thread t adds parts[t], parts[t + 256], ..; then the tree
inline double pcg_block_sum(const double* parts, uint32_t n) {
  double v[256];
  for (uint32_t t = 0; t < 256; ++t) {
    double s = 0.0;
    for (uint32_t i = t; i < n; i += 256) s += parts[i];
    v[t] = s;
  }
  return pcg_tree(v, 256);
}

PCG_HD inline bool pcg_finite(double v) { return v - v == 0.0; }

// C = Z^T S Z as k_pcg_coarse_assemble forms it: C (ncp x ncp, row-major, both triangles; the padding is the
// identity).  Entry (a, b), a >= b, is the sum of S(i, j) over the fine rows i of a, then the fine rows j of b, in
// list order; S(i, j) is read from the lower storage at (max, min), of the pattern's tiles only (others count 0).
inline void pcg_coarse_assemble_host(const PcgPlan& pl, const double* A, size_t ld, const std::vector<uint8_t>& nz,
                                     std::vector<double>& C) {
  const uint32_t ncp = pl.ncp, nt = pl.nt;
  C.assign((size_t)ncp * ncp, 0.0);
  for (uint32_t a = 0; a < ncp; ++a)
    for (uint32_t b = 0; b <= a; ++b) {
      double sum = 0.0;
      bool empty = true;
      if (a < pl.nc) {
        empty = pl.crow_ptr[a] == pl.crow_ptr[a + 1];
        for (uint32_t x = pl.crow_ptr[a]; x < pl.crow_ptr[a + 1]; ++x)
          for (uint32_t y = pl.crow_ptr[b]; y < pl.crow_ptr[b + 1]; ++y) {
            const uint32_t i = pl.crow_rows[x], j = pl.crow_rows[y];
            const uint32_t r = std::max(i, j), c = std::min(i, j);
            if (r / 64 == c / 64 || nz[(size_t)(r / 64) * nt + c / 64]) sum += A[(size_t)r * ld + c];
          }
      }
      if (empty && a == b) sum = 1.0;
      C[(size_t)a * ncp + b] = sum;
      C[(size_t)b * ncp + a] = sum;
    }
}

// Cholesky factor of a 64 x 64 tile held in d[64][65] (lower triangle) and, in the strict upper triangle, the
// transpose of its inverse W = L^-1 (W[r][c] at d[c][r]); dinv[c] = 1 / L[c][c] = W[c][c].  A pivot that is not
// positive and finite gives a zero column and returns false (k_pcg_coarse_column runs the same steps in LDS).
inline bool pcg_coarse_tile_factor(double (*d)[65], double* dinv) {
  bool ok = true;
  for (uint32_t j = 0; j < 64; ++j) {
    const double p = d[j][j];
    const bool good = p > 0.0 && std::isfinite(p);
    if (!good) ok = false;
    const double l = good ? std::sqrt(p) : 0.0, il = good ? 1.0 / l : 0.0;
    d[j][j] = l;
    dinv[j] = il;
    for (uint32_t r = j + 1; r < 64; ++r) d[r][j] *= il;
    for (uint32_t r = j + 1; r < 64; ++r)
      for (uint32_t c = j + 1; c <= r; ++c) d[r][c] -= d[r][j] * d[c][j];
  }
  for (uint32_t c = 0; c < 64; ++c)
    for (uint32_t r = c + 1; r < 64; ++r) {
      double s = d[r][c] * dinv[c];
      for (uint32_t m = c + 1; m < r; ++m) s += d[r][m] * d[c][m];
      d[c][r] = -s * dinv[r];
    }
  return ok;
}

// Explicit symmetric C^-1 (ncp x ncp) by the steps of k_pcg_coarse.hip: left-looking blocked Cholesky on 64-tiles
// (L_ik = (C_ik - sum_m L_im L_km^T) W_kk^T with W_kk = L_kk^-1), W = L^-1 tile column by tile column, then
// C^-1 = W^T W with the diagonal tiles symmetrised and the upper tiles mirrored.  Returns false on a bad pivot.
inline bool pcg_coarse_invert_host(const std::vector<double>& C, uint32_t ncp, std::vector<double>& Cinv) {
  const uint32_t nct = ncp / 64;
  const size_t N = ncp;
  std::vector<double> L((size_t)ncp * ncp, 0.0), W((size_t)ncp * ncp, 0.0), T(64 * 64);
  Cinv.assign((size_t)ncp * ncp, 0.0);
  bool ok = true;
  for (uint32_t k = 0; k < nct; ++k) {
    static thread_local double d[64][65];
    double dinv[64];
    for (uint32_t r = 0; r < 64; ++r)
      for (uint32_t c = 0; c < 64; ++c) {
        double s = 0.0;
        for (uint32_t m = 0; m < 64 * k; ++m) s += L[(64 * k + r) * N + m] * L[(64 * k + c) * N + m];
        d[r][c] = C[(64 * k + r) * N + 64 * k + c] - s;
      }
    if (!pcg_coarse_tile_factor(d, dinv)) ok = false;
    for (uint32_t r = 0; r < 64; ++r)
      for (uint32_t c = 0; c < 64; ++c) {
        L[(64 * k + r) * N + 64 * k + c] = c <= r ? d[r][c] : 0.0;
        W[(64 * k + r) * N + 64 * k + c] = c < r ? d[c][r] : c == r ? dinv[c] : 0.0;
      }
    for (uint32_t i = k + 1; i < nct; ++i) {
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t c = 0; c < 64; ++c) {
          double s = 0.0;
          for (uint32_t m = 0; m < 64 * k; ++m) s += L[(64 * i + r) * N + m] * L[(64 * k + c) * N + m];
          T[r * 64 + c] = C[(64 * i + r) * N + 64 * k + c] - s;
        }
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t c = 0; c < 64; ++c) {
          double s = 0.0;
          for (uint32_t m = 0; m <= c; ++m) s += T[r * 64 + m] * W[(64 * k + c) * N + 64 * k + m];
          L[(64 * i + r) * N + 64 * k + c] = s;
        }
    }
  }
  for (uint32_t k = 0; k < nct; ++k)
    for (uint32_t i = k + 1; i < nct; ++i) {
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t c = 0; c < 64; ++c) {
          double s = 0.0;
          for (uint32_t m = 64 * k; m < 64 * i; ++m) s += L[(64 * i + r) * N + m] * W[m * N + 64 * k + c];
          T[r * 64 + c] = s;
        }
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t c = 0; c < 64; ++c) {
          double s = 0.0;
          for (uint32_t m = 0; m < 64; ++m) s += W[(64 * i + r) * N + 64 * i + m] * T[m * 64 + c];
          W[(64 * i + r) * N + 64 * k + c] = -s;
        }
    }
  for (uint32_t i = 0; i < nct; ++i)
    for (uint32_t j = 0; j <= i; ++j) {
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t c = 0; c < 64; ++c) {
          double s = 0.0;
          for (uint32_t m = 64 * i; m < ncp; ++m) s += W[m * N + 64 * i + r] * W[m * N + 64 * j + c];
          T[r * 64 + c] = s;
        }
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t c = 0; c < 64; ++c) {
          if (i == j) Cinv[(64 * i + r) * N + 64 * j + c] = 0.5 * (T[r * 64 + c] + T[c * 64 + r]);
          else Cinv[(64 * i + r) * N + 64 * j + c] = Cinv[(64 * j + c) * N + 64 * i + r] = T[r * 64 + c];
        }
    }
  return ok;
}

// y_c = C^-1 r_c and the per-row partials of r_c . y_c as k_pcg_coarse_apply forms them: 64 lanes per row, lane t
// sums the columns t, t + 64, ..; then the tree.
inline void pcg_coarse_apply_host(const std::vector<double>& Cinv, uint32_t nc, uint32_t ncp, const double* rc, double* yc,
                                  double* part) {
  for (uint32_t row = 0; row < nc; ++row) {
    double v[64];
    for (uint32_t t = 0; t < 64; ++t) {
      double s = 0.0;
      for (uint32_t m = t; m < ncp; m += 64) s += Cinv[(size_t)row * ncp + m] * rc[m];
      v[t] = s;
    }
    yc[row] = pcg_tree(v, 64);
    part[row] = rc[row] * yc[row];
  }
}

// The decision of one pass from its three sums (pq = p.Sp, rz = r.z, rr = r.r of the NEW residual).  `out` is the
// next state; the return value says what update2 does to x and p.  Stopping rule: when the recurrence passes
// ||r|| <= tol ||b|| the next pass recomputes r = b - S x (kPcgVerify) and only that residual ends the solve; if it
// fails, the solve continues from the recomputed residual with p = z (residual replacement).  Breakdown: 1 = p.Sp
// <= 0, 2 = a non-finite scalar, 3 = a preconditioner block that is not positive definite (bit 0 of block_status),
// 4 = a coarse matrix that is not positive definite (bit 1; 3 wins when both are set); x is not moved by the
// pass that detects it.  max_it counts CG steps; reaching it ends the solve with converged = 0.
PCG_HD inline uint32_t pcg_decide(const PcgState& s, double pq, double rz, double rr, int block_status, PcgState& out,
                                  double& alpha, double& beta) {
  out = s;
  alpha = beta = 0.0;
  if (s.done) return 0;
  if (s.mode != kPcgIter) {
    if (s.mode == kPcgInit && block_status) { out.done = 1; out.breakdown = (block_status & 1) ? 3 : 4; return 0; }
    if (!pcg_finite(rr) || !pcg_finite(rz)) { out.done = 1; out.breakdown = 2; return 0; }
    if (s.mode == kPcgInit) {
      out.bb = rr;
      out.rr_recur = rr;
      if (rr == 0.0) { out.done = 1; out.converged = 1; out.rr_true = 0.0; return 0; }
    } else {
      out.rr_true = rr;
      if (rr <= s.tol2 * s.bb) { out.done = 1; out.converged = 1; return 0; }
      out.replacements = s.replacements + 1;
      out.rr_recur = rr;
      if (s.iterations >= s.max_it) { out.done = 1; return 0; }
    }
    out.rz_old = rz;
    out.mode = kPcgIter;
    return kPcgRestart;
  }
  if (!pcg_finite(pq)) { out.done = 1; out.breakdown = 2; return 0; }
  if (pq <= 0.0) { out.done = 1; out.breakdown = 1; return 0; }
  alpha = s.rz_old / pq;
  if (!pcg_finite(alpha) || !pcg_finite(rr) || !pcg_finite(rz)) { out.done = 1; out.breakdown = 2; alpha = 0.0; return 0; }
  out.iterations = s.iterations + 1;
  out.rr_recur = rr;
  if (rr <= s.tol2 * s.bb) { out.mode = kPcgVerify; return kPcgStep; }
  if (out.iterations >= s.max_it) { out.done = 1; return kPcgStep; }
  beta = rz / s.rz_old;
  out.rz_old = rz;
  return kPcgStep | kPcgDir;
}

// q = S v as k_pcg_spmv_tiles + k_pcg_spmv_gather form it.  A: lower storage, row-major, leading dimension ld >=
// 64 nt; only the tiles of the plan are read, of a diagonal tile only the lower triangle.  v, q: 64 nt.
// Inside a tile: thread (rg, c2), rg = 0..7, c2 = 0..31, owns the columns 2 c2, 2 c2 + 1 of the rows rg + 8 k.
inline void pcg_spmv_host(const PcgPlan& pl, const double* A, size_t ld, const double* v, double* q,
                          std::vector<double>& rowslot, std::vector<double>& colslot) {
  rowslot.assign((size_t)pl.n_tiles * 64, 0.0);
  colslot.assign((size_t)pl.n_tiles * 64, 0.0);
  for (uint32_t s = 0; s < pl.n_tiles; ++s) {
    const uint32_t I = pl.tiles[2 * s], J = pl.tiles[2 * s + 1];
    const bool diag = I == J;
    const double* T = A + (size_t)I * 64 * ld + (size_t)J * 64;
    const double* vI = v + (size_t)I * 64;
    const double* vJ = v + (size_t)J * 64;
    for (uint32_t r = 0; r < 64; ++r) {
      double sum = 0.0;
      for (uint32_t c2 = 0; c2 < 32; ++c2) {
        const uint32_t c = 2 * c2;
        const double a0 = diag && c > r ? 0.0 : T[(size_t)r * ld + c];
        const double a1 = diag && c + 1 > r ? 0.0 : T[(size_t)r * ld + c + 1];
        sum += a0 * vJ[c] + a1 * vJ[c + 1];
      }
      rowslot[(size_t)s * 64 + r] = sum;
    }
    for (uint32_t c = 0; c < 64; ++c) {
      double sum = 0.0;
      for (uint32_t rg = 0; rg < 8; ++rg) {
        double part = 0.0;
        for (uint32_t k = 0; k < 8; ++k) {
          const uint32_t r = rg + 8 * k;
          const double a = diag && c >= r ? 0.0 : T[(size_t)r * ld + c];
          part += a * vI[r];
        }
        sum += part;
      }
      colslot[(size_t)s * 64 + c] = sum;
    }
  }
  for (uint32_t I = 0; I < pl.nt; ++I)
    for (uint32_t t = 0; t < 64; ++t) {
      double sum = 0.0;
      for (uint32_t s = pl.row_ptr[I]; s < pl.row_ptr[I + 1]; ++s) sum += rowslot[(size_t)s * 64 + t];
      for (uint32_t e = pl.col_ptr[I]; e < pl.col_ptr[I + 1]; ++e) sum += colslot[(size_t)pl.col_slot[e] * 64 + t];
      q[(size_t)I * 64 + t] = sum;
    }
}

// M^-1 of every block of `blocks` ((start, size) pairs) from the lower storage A; minv: 16 doubles per row of
// the padded system (row r of its block's inverse).  Elements of tiles outside nz count as zero.  Returns the
// status word of k_pcg_blocks: 1 if some block is not positive definite.
inline int pcg_blocks_host(const double* A, size_t ld, const std::vector<uint8_t>& nz, uint32_t nt,
                           const std::vector<uint32_t>& blocks, std::vector<double>& minv) {
  minv.assign(ld * 16, 0.0);
  int status = 0;
  for (size_t b = 0; b < blocks.size(); b += 2) {
    const uint32_t start = blocks[b], D = blocks[b + 1];
    double a[256] = {0.0};
    for (uint32_t i = 0; i < D; ++i)
      for (uint32_t j = 0; j < D; ++j) {
        const uint32_t r = start + std::max(i, j), c = start + std::min(i, j);
        const bool on = r / 64 == c / 64 || nz[(size_t)(r / 64) * nt + c / 64];
        a[i * 16 + j] = on ? A[(size_t)r * ld + c] : 0.0;
      }
    if (!pcg_invert_block(a, D)) status = 1;
    for (uint32_t i = 0; i < D; ++i)
      for (uint32_t j = 0; j < D; ++j) minv[(size_t)(start + i) * 16 + j] = 0.5 * (a[i * 16 + j] + a[j * 16 + i]);
  }
  return status;
}

struct PcgResult {
  uint32_t iterations = 0, converged = 0, replacements = 0, breakdown = 0, passes = 0;
  double rr_recur = 0.0, rr_true = 0.0, bb = 0.0;
};

inline uint32_t pcg_max_passes(uint32_t max_it) { return 2 * max_it + 3; }

// The solver, pass by pass as the device runs it.  n: unknowns (rows n .. ld are padding: identity rows of A,
// zero rhs); x: ld doubles.  Returns 0, or 4 (BA_HIP_FACTORIZATION_ERROR) on a breakdown.
inline int pcg_host(const PcgPlan& pl, const double* A, size_t ld, const double* rhs, uint32_t n,
                    const std::vector<uint8_t>& nz, const std::vector<uint32_t>& blk, const std::vector<uint32_t>& blocks,
                    double rel_tolerance, uint32_t max_it, double* x, PcgResult* res, bool coarse = false,
                    std::vector<double>* C_out = nullptr, std::vector<double>* Cinv_out = nullptr) {
  std::vector<double> minv, rowslot, colslot, r[2], z(ld, 0.0), p(ld, 0.0), q(ld, 0.0);
  r[0].assign(ld, 0.0);
  r[1].assign(ld, 0.0);
  int block_status = pcg_blocks_host(A, ld, nz, pl.nt, blocks, minv);
  std::vector<double> C, Cinv, rc, yc, ryc_part;
  if (coarse) {   // the plan carries build_pcg_coarse's tables
    pcg_coarse_assemble_host(pl, A, ld, nz, C);
    if (!pcg_coarse_invert_host(C, pl.ncp, Cinv)) block_status |= 2;
    rc.assign(pl.ncp, 0.0);
    yc.assign(pl.ncp, 0.0);
    ryc_part.assign(pl.nc, 0.0);
    if (C_out) *C_out = C;
    if (Cinv_out) *Cinv_out = Cinv;
  }
  std::fill(x, x + ld, 0.0);
  PcgState st[2] = {};
  st[0].tol2 = rel_tolerance * rel_tolerance;
  st[0].max_it = max_it ? max_it : n;
  st[0].mode = kPcgInit;
  const uint32_t nb = (uint32_t)((ld + 255) / 256);
  std::vector<double> pq_part(pl.nt, 0.0), rz_part(nb, 0.0), rr_part(nb, 0.0);
  uint32_t k = 0;
  for (; k < pcg_max_passes(st[0].max_it); ++k) {
    const PcgState& s = st[k & 1];
    if (s.done) break;
    const std::vector<double>& rin = r[k & 1];
    std::vector<double>& rout = r[(k + 1) & 1];
    double alpha1 = 0.0;
    bool run1 = true;
    if (s.mode != kPcgInit) {
      pcg_spmv_host(pl, A, ld, s.mode == kPcgVerify ? x : p.data(), q.data(), rowslot, colslot);
      for (uint32_t I = 0; I < pl.nt; ++I) {
        double v[64];
        for (uint32_t t = 0; t < 64; ++t) v[t] = p[(size_t)I * 64 + t] * q[(size_t)I * 64 + t];
        pq_part[I] = pcg_tree(v, 64);
      }
    }
    if (s.mode == kPcgIter) {   // update1 forms alpha itself; an unusable one makes the whole launch a no-op
      const double pq = pcg_block_sum(pq_part.data(), pl.nt);
      alpha1 = s.rz_old / pq;
      run1 = pcg_finite(pq) && pq > 0.0 && pcg_finite(alpha1);
    }
    if (run1)
      for (uint32_t b = 0; b < nb; ++b) {
        double vz[256], vr[256];
        for (uint32_t t = 0; t < 256; ++t) {
          const size_t row = (size_t)b * 256 + t;
          double rn = 0.0, zz = 0.0;
          if (row < n) {
            const uint32_t start = blk[2 * row], D = blk[2 * row + 1];
            for (uint32_t j = 0; j < D; ++j) {
              const size_t c = start + j;
              const double rj = s.mode == kPcgIter ? rin[c] - alpha1 * q[c] : s.mode == kPcgInit ? rhs[c] : rhs[c] - q[c];
              if (c == row) rn = rj;
              zz += minv[row * 16 + j] * rj;
            }
          }
          if (row < ld) { rout[row] = rn; z[row] = zz; }
          vz[t] = rn * zz;
          vr[t] = rn * rn;
        }
        rz_part[b] = pcg_tree(vz, 256);
        rr_part[b] = pcg_tree(vr, 256);
      }
    if (run1 && coarse) {
      for (uint32_t c = 0; c < pl.nc; ++c) {
        double sum = 0.0;
        for (uint32_t e = pl.crow_ptr[c]; e < pl.crow_ptr[c + 1]; ++e) sum += rout[pl.crow_rows[e]];
        rc[c] = sum;
      }
      pcg_coarse_apply_host(Cinv, pl.nc, pl.ncp, rc.data(), yc.data(), ryc_part.data());
    }
    const double pq = s.mode == kPcgIter ? pcg_block_sum(pq_part.data(), pl.nt) : 0.0;
    double rz = pcg_block_sum(rz_part.data(), nb);
    const double rr = pcg_block_sum(rr_part.data(), nb);
    if (coarse) rz += pcg_block_sum(ryc_part.data(), pl.nc);
    double alpha, beta;
    const uint32_t act = pcg_decide(s, pq, rz, rr, block_status, st[(k + 1) & 1], alpha, beta);
    for (size_t row = 0; row < ld; ++row) {
      const double zr = coarse && pl.cmap[row] != kPcgNone ? z[row] + yc[pl.cmap[row]] : z[row];
      if (act & kPcgStep) x[row] += alpha * p[row];
      if (act & kPcgDir) p[row] = zr + beta * p[row];
      else if (act & kPcgRestart) p[row] = zr;
    }
  }
  const PcgState& f = st[k & 1];
  if (res) {
    res->iterations = f.iterations; res->converged = f.converged; res->replacements = f.replacements;
    res->breakdown = f.breakdown; res->passes = k; res->rr_recur = f.rr_recur; res->rr_true = f.rr_true; res->bb = f.bb;
  }
  return f.breakdown ? 4 : 0;
}

}  // namespace bae
