// Marginal covariances of poses, calibration and landmarks by selected inversion of the factor that
// ba_hip_solve_gn leaves behind (ba_hip_compute_marginals and the ba_hip_get_*_marginals readers).
//
//   k_selinv_col   Sigma_IJ = -(sum_{K in R_J} Sigma_IK L_KJ) L_JJ^-1, one workgroup per (J, I in R_J)
//   k_selinv_diag  Sigma_JJ = (L_JJ^-T D_J - sum_{K in R_J} Sigma_KJ^T L_KJ) L_JJ^-1, one workgroup per J
//   k_selinv_gather   D x D / K x K blocks out of the compact store
//   k_selinv_lm_*  Sigma_ll = V^-1 + V^-1 (sum_{a,b} W_a^T Sigma_{p_a p_b} W_b) V^-1, one wavefront per landmark
//
// The recursion, the compact store and the level schedule are in selinv.h (host restatement:
// selinv_host, checked on the CPU by tests/test_selected_inverse.py).  The factor is read, never
// written: L_KJ from A, L_JJ^-T (linvT) and the pivot signs D from invdiag.  k_selinv_diag reads the
// Sigma_KJ its column's k_selinv_col launch wrote, so it is a second launch.
//
// The tile products run on v_mfma_f64_16x16x4_f64 with the staging and the 4-wave 2x2 layout of tile_mma.h.
#include "engine.h"
#include "selinv.h"
#include "tile_mma.h"
#include "lm_entry.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace bae {

using namespace tile64;

namespace {

__device__ __forceinline__ const double* slot_tile(const double* store, const uint32_t* slot, uint32_t nt, uint32_t i,
                                                   uint32_t k) {
  return store + (size_t)slot[(size_t)i * nt + k] * (TB * TB);
}

// The K loop of both kernels: acc = sum over the tiles K of R_J (2 chunks each) of  A_K x L_KJ, where the
// A operand is Sigma_IK (COL, I >= K: index-major slot (I, K); I < K: k-major slot (K, I)) or Sigma_KJ^T
// (DIAG: k-major slot (K, J)).  B = L_KJ from A (k-major).
template <bool DIAG>
__device__ __forceinline__ void k_loop(double4_t (&acc)[2][2], Lds& s, uint32_t I, uint32_t J, const uint32_t* R,
                                       uint32_t m, const double* __restrict__ A, size_t ld,
                                       const uint32_t* __restrict__ slot, uint32_t nt,
                                       const double* __restrict__ store) {
  Chunk ca, cb;
  bool a_imajor = false;
  auto fetch = [&](uint32_t ch) {
    const uint32_t K = R[ch >> 1];
    const int k0 = KCH * (int)(ch & 1);
    if (DIAG) {
      a_imajor = false;
      load_kmajor(ca, slot_tile(store, slot, nt, K, J), TB, k0);
    } else if (I >= K) {
      a_imajor = true;
      load_imajor(ca, slot_tile(store, slot, nt, I, K), TB, k0);
    } else {
      a_imajor = false;
      load_kmajor(ca, slot_tile(store, slot, nt, K, I), TB, k0);
    }
    load_kmajor(cb, A + (size_t)K * TB * ld + (size_t)J * TB, ld, k0);
  };
  accumulate_chunks(acc, s, 2 * m, fetch, [&](uint32_t) {
    if (a_imajor) store_imajor(ca, s.X);
    else store_kmajor(ca, s.X);
    store_kmajor(cb, s.Y);
  });
}

// Epilogue product: out = M x L_JJ^-1 with M[r][x] = sgn * T[r][x] (+ L_JJ^-T[r][x] d_x when DIAG), T in acc.
// B[x][c] = (L_JJ^-1)[x][c] = linvT[c][x]: an index-major source.
template <bool DIAG>
__device__ __forceinline__ void epilogue(double4_t (&out)[2][2], const double4_t (&acc)[2][2], Lds& s,
                                         const double* __restrict__ G, const double* __restrict__ dsgn) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int rb = 32 * (wave >> 1), cb = 32 * (wave & 1);
  zero_acc(out);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    // columns x in [32 h, 32 h + 32) of T belong to the waves with cb == 32 h
    if (cb == KCH * h) {
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int r = rb + 16 * ti + lk + 4 * reg, x = 16 * tj + li;
            s.X[x][r] = -acc[ti][tj][reg];
          }
    }
    Chunk cg;
    load_imajor(cg, G, TB, KCH * h);
    store_imajor(cg, s.Y);
    __syncthreads();
    if (DIAG) {
      // + L_JJ^-T D: X[x][r] += G[r][32 h + x] d_{32 h + x}
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int e = tid + 256 * q, x = e % KCH, r = e / KCH;
        s.X[x][r] += G[(size_t)r * TB + KCH * h + x] * dsgn[KCH * h + x];
      }
      __syncthreads();
    }
    mma_chunk(out, s);
    __syncthreads();
  }
}

}  // namespace

// items: (J, I) pairs of one level; Sigma_IJ = -(sum_K Sigma_IK L_KJ) L_JJ^-1
__global__ void __launch_bounds__(256)
k_selinv_col(const uint2* __restrict__ items, const uint32_t* __restrict__ col_ptr,
             const uint32_t* __restrict__ col_rows, const double* __restrict__ A, uint32_t ld,
             const double* __restrict__ linvT, const uint32_t* __restrict__ slot, uint32_t nt,
             double* __restrict__ store) {
  __shared__ Lds s;
  const uint2 it = items[blockIdx.x];
  const uint32_t J = it.x, I = it.y;
  const uint32_t* R = col_rows + col_ptr[J];
  const uint32_t m = col_ptr[J + 1] - col_ptr[J];
  double4_t acc[2][2], out[2][2];
  zero_acc(acc);
  k_loop<false>(acc, s, I, J, R, m, A, ld, slot, nt, store);
  epilogue<false>(out, acc, s, linvT + (size_t)J * TB * TB, nullptr);
  store_tile(store + (size_t)slot[(size_t)I * nt + J] * TB * TB, TB, out);
}

// cols: the columns J of one level; Sigma_JJ = (L_JJ^-T D_J - sum_K Sigma_KJ^T L_KJ) L_JJ^-1
__global__ void __launch_bounds__(256)
k_selinv_diag(const uint32_t* __restrict__ cols, const uint32_t* __restrict__ col_ptr,
              const uint32_t* __restrict__ col_rows, const double* __restrict__ A, uint32_t ld,
              const double* __restrict__ linvT, const double* __restrict__ dsgn,
              const uint32_t* __restrict__ slot, uint32_t nt, double* __restrict__ store) {
  __shared__ Lds s;
  const uint32_t J = cols[blockIdx.x];
  const uint32_t* R = col_rows + col_ptr[J];
  const uint32_t m = col_ptr[J + 1] - col_ptr[J];
  double4_t acc[2][2], out[2][2];
  zero_acc(acc);
  k_loop<true>(acc, s, J, J, R, m, A, ld, slot, nt, store);
  epilogue<true>(out, acc, s, linvT + (size_t)J * TB * TB, dsgn + (size_t)J * TB);
  store_tile(store + (size_t)slot[(size_t)J * nt + J] * TB * TB, TB, out);
}

// out[q][i][j] = Sigma[ra[q] + i][rb[q] + j], i < Da, j < Db
__global__ void __launch_bounds__(256)
k_selinv_gather(uint32_t n, const uint32_t* __restrict__ ra, const uint32_t* __restrict__ rb, int Da, int Db,
                const uint32_t* __restrict__ slot, uint32_t nt, const double* __restrict__ store,
                double* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t per = (uint64_t)Da * Db;
  if (t >= (uint64_t)n * per) return;
  const uint32_t q = (uint32_t)(t / per), e = (uint32_t)(t % per);
  out[t] = sig_at(store, slot, nt, ra[q] + e / Db, rb[q] + e % Db);
}

// ---- landmark blocks (LmArgs, lm_entry: lm_entry.h) ------------------------------------------------------
// Sigma_ll of landmark l by the calling wavefront (all 64 lanes); lane 0 writes LM x LM values to out.
// Lane j takes the entry pairs j, j + 64, ... in a fixed order and the partial sums meet in a fixed
// butterfly: the result does not depend on which launch or wavefront computes the landmark.
template <int LM>
__device__ void lm_sigma(const LmArgs& g, uint32_t l, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const uint32_t nobs = g.lm_ptr[l + 1] - g.lm_ptr[l];
  bool any_listed = false;
  if (LM == 1) {
    const uint32_t rp = g.lm_ref_pose[l];
    for (uint32_t e0 = 0; e0 < nobs; e0 += 64) {
      const uint32_t e = e0 + lane;
      const bool lst = e < nobs && g.obs_pose[g.lm_ptr[l] + e] != rp;
      any_listed = any_listed || __ballot(lst) != 0;
    }
  }
  const uint32_t ne = nobs + (LM == 1 ? 1u : 0u) + (g.K > 0 ? 1u : 0u);
  double U[LM][LM];
#pragma unroll
  for (int a = 0; a < LM; ++a)
#pragma unroll
    for (int b = 0; b < LM; ++b) U[a][b] = 0.0;
  const uint64_t npairs = (uint64_t)ne * ne;
  for (uint64_t q = lane; q < npairs; q += 64) {
    const LmEntry<LM> ea = lm_entry<LM>(g, l, (uint32_t)(q / ne), nobs, any_listed);
    const LmEntry<LM> eb = lm_entry<LM>(g, l, (uint32_t)(q % ne), nobs, any_listed);
    if (!ea.valid || !eb.valid) continue;
    // v[i][k2] = sum_j Sigma[a + i][b + j] w_b[k2][j]
    // (fixed trip counts with guards: the arrays stay in registers)
    double v[6][LM];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int k = 0; k < LM; ++k) v[i][k] = 0.0;
      if (i < ea.width) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          if (j < eb.width) {
            const double sg = sig_at(g.store, g.slot, g.nt, ea.base + i, eb.base + j);
#pragma unroll
            for (int k = 0; k < LM; ++k) v[i][k] += sg * eb.w[k * kRow + j];
          }
        }
      }
    }
#pragma unroll
    for (int k1 = 0; k1 < LM; ++k1)
#pragma unroll
      for (int k2 = 0; k2 < LM; ++k2) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
          if (i < ea.width) s += ea.w[k1 * kRow + i] * v[i][k2];
        U[k1][k2] += s;
      }
  }
#pragma unroll
  for (int a = 0; a < LM; ++a)
#pragma unroll
    for (int b = 0; b < LM; ++b) {
      double u = U[a][b];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) u += __shfl_xor(u, off, 64);
      U[a][b] = u;
    }
  if (lane == 0) {
    // a landmark without observations is in no linearisation range: k_linearize never wrote its V^-1 (the buffer
    // holds zeros there).  Its V is zero and the guard of invert_v (BundleAdjuster.cpp:431-439) makes it 1e-6 I.
    double Vi[LM * LM];
#pragma unroll
    for (int a = 0; a < LM * LM; ++a) Vi[a] = nobs ? g.lm_vinv[(size_t)l * LM * LM + a] : (a % (LM + 1) == 0 ? 1e6 : 0.0);
    double T[LM][LM];
#pragma unroll
    for (int a = 0; a < LM; ++a)
#pragma unroll
      for (int b = 0; b < LM; ++b) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < LM; ++c) s += U[a][c] * Vi[c * LM + b];
        T[a][b] = s;
      }
#pragma unroll
    for (int a = 0; a < LM; ++a)
#pragma unroll
      for (int b = 0; b < LM; ++b) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < LM; ++c) s += Vi[a * LM + c] * T[c][b];
        out[a * LM + b] = Vi[a * LM + b] + s;
      }
  }
}

// requested landmarks: one wavefront per id (ids checked on the host)
template <int LM>
__global__ void __launch_bounds__(256) k_selinv_lm_ids(LmArgs g, uint32_t n, const uint32_t* __restrict__ ids,
                                                       double* __restrict__ out) {
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n) return;
  lm_sigma<LM>(g, ids[q], out + (size_t)q * LM * LM);
}

// every active landmark: one wavefront per linearisation range (wave_rng: whole landmarks, at most 64
// observations, or one landmark with more); output by optimisation index, like delta_l
template <int LM>
__global__ void __launch_bounds__(256) k_selinv_lm_ranges(LmArgs g, uint32_t n_rng, const uint2* __restrict__ rng,
                                                          double* __restrict__ out) {
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_rng) return;
  const uint2 r = rng[q];
  if (r.y <= r.x) return;
  const uint32_t l0 = g.obs_lm[r.x], l1 = g.obs_lm[r.y - 1];
  // landmarks without observations inside the span belong to k_selinv_lm_bare
  for (uint32_t l = l0; l <= l1; ++l)
    if (g.lm_opt[l] >= 0 && g.lm_ptr[l + 1] > g.lm_ptr[l]) lm_sigma<LM>(g, l, out + (size_t)g.lm_opt[l] * LM * LM);
}

// active landmarks without observations (in no range): Sigma_ll = V^-1 (+ the calibration term)
template <int LM>
__global__ void __launch_bounds__(256) k_selinv_lm_bare(LmArgs g, uint32_t L, double* __restrict__ out) {
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= L) return;
  if (g.lm_opt[q] < 0 || g.lm_ptr[q + 1] != g.lm_ptr[q]) return;
  lm_sigma<LM>(g, q, out + (size_t)g.lm_opt[q] * LM * LM);
}

// ---- host side ----------------------------------------------------------------------------------------
int marginals_compute(Engine* e) {
  const Structure& st = e->st;
  if (e->held.sig_valid) return 0;
  uint32_t nt;
  const double *dsgn, *linvT;
  int rc;
  if ((rc = kept_factor(e, "marginals", &nt, &dsgn, &linvT))) return rc;
  if (e->sig_plan_version != e->nzL_version) {
    build_selinv_plan(e->nzL_host, nt, e->sig_plan);
    const SelinvPlan& p = e->sig_plan;
    // the tables are members of e->sig_plan and the kernels that read them run on the same stream
    if ((rc = upload_async(e, e->sig_slot, p.slot.data(), p.slot.size())) ||
        (rc = upload_async(e, e->sig_col_ptr, p.col_ptr.data(), p.col_ptr.size())) ||
        (rc = upload_async(e, e->sig_col_rows, p.col_rows.data(), p.col_rows.size())) ||
        (rc = upload_async(e, e->sig_level_cols, p.level_cols.data(), p.level_cols.size())) ||
        (rc = upload_async(e, e->sig_items, p.items.data(), p.items.size())))
      return rc;
    e->sig_plan_version = e->nzL_version;
  }
  const SelinvPlan& p = e->sig_plan;
  const size_t count = (size_t)p.n_slots * TB * TB;
  if (e->sig.n < count) {
    e->sig.release();   // (before the larger store is allocated: lowers the peak)
    const hipError_t err = e->sig.alloc(count);
    if (err != hipSuccess) {
      (void)hipGetLastError();
      char msg[160];
      snprintf(msg, sizeof msg, "marginals: allocating the selected-inverse store (%zu bytes, %u tiles) failed",
               count * sizeof(double), p.n_slots);
      return e->fail_msg(msg);
    }
  }
  Events<2> ev;
  BAE_HIP(ev.create());
  (void)ev.record(0, e->stream);
  const uint32_t levels = (uint32_t)p.level_ptr.size() - 1;
  for (uint32_t v = 0; v < levels; ++v) {
    const uint32_t i0 = p.item_ptr[v], i1 = p.item_ptr[v + 1];
    if (i1 > i0)
      hipLaunchKernelGGL(k_selinv_col, dim3(i1 - i0), dim3(256), 0, e->stream,
                         reinterpret_cast<const uint2*>(e->sig_items.p) + i0, (const uint32_t*)e->sig_col_ptr.p,
                         (const uint32_t*)e->sig_col_rows.p, (const double*)e->A.p, st.ld, linvT,
                         (const uint32_t*)e->sig_slot.p, nt, e->sig.p);
    const uint32_t c0 = p.level_ptr[v], c1 = p.level_ptr[v + 1];
    hipLaunchKernelGGL(k_selinv_diag, dim3(c1 - c0), dim3(256), 0, e->stream, (const uint32_t*)e->sig_level_cols.p + c0,
                       (const uint32_t*)e->sig_col_ptr.p, (const uint32_t*)e->sig_col_rows.p, (const double*)e->A.p,
                       st.ld, linvT, dsgn, (const uint32_t*)e->sig_slot.p, nt, e->sig.p);
  }
  (void)ev.record(1, e->stream);
  const hipError_t lerr = hipGetLastError();
  const hipError_t serr = hipEventSynchronize(ev[1]);
  e->mstats.selinv_ms = ev.ms(0, 1);
  if (lerr != hipSuccess) return e->fail(lerr, "k_selinv launch");
  if (serr != hipSuccess) return e->fail(serr, "k_selinv");
  e->mstats.tile_products = p.products;
  e->mstats.factor_tile_products = factor_tile_products(e->nzL_host, nt);
  e->mstats.store_bytes = (double)count * sizeof(double);
  e->mstats.levels = levels;
  e->mstats.store_tiles = p.n_slots;
  e->held.selinv_computed();
  return 0;
}

int marginals_gather(Engine* e, uint32_t n, const std::vector<uint32_t>& ra, const std::vector<uint32_t>& rb, int Da,
                     int Db, double* out) {
  if (n == 0) return 0;
  const uint32_t nt = e->st.ld / TB;
  // every tile the blocks touch must lie in the pattern
  for (uint32_t q = 0; q < n; ++q)
    for (uint32_t t1 = ra[q] / TB; t1 <= (ra[q] + Da - 1) / TB; ++t1)
      for (uint32_t t2 = rb[q] / TB; t2 <= (rb[q] + Db - 1) / TB; ++t2) {
        const uint32_t hi = std::max(t1, t2), lo = std::min(t1, t2);
        if (e->sig_plan.slot[(size_t)hi * nt + lo] == kNoSlot)
          return e->fail_msg("marginals: the requested block lies outside the factor's tile pattern (the two poses share "
                             "no landmark and no pose-pose residual, and no fill couples them)");
      }
  DBuf<uint32_t> d;
  DBuf<double> o;
  BAE_HIP(d.alloc(2 * (size_t)n));
  const size_t cnt = (size_t)n * Da * Db;
  if (o.alloc(cnt) != hipSuccess) return e->fail_msg("marginals: output allocation failed");
  hipError_t err = hipMemcpy(d.p, ra.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(d.p + n, rb.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_selinv_gather, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, e->stream, n,
                       (const uint32_t*)d.p, (const uint32_t*)d.p + n, Da, Db, (const uint32_t*)e->sig_slot.p, nt,
                       (const double*)e->sig.p, o.p);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess) err = hipMemcpy(out, o.p, cnt * sizeof(double), hipMemcpyDeviceToHost);
  return err == hipSuccess ? 0 : e->fail(err, "k_selinv_gather");
}

int marginals_landmarks(Engine* e, uint32_t n, const uint32_t* ids, double* out) {
  const Structure& st = e->st;
  const int LM = e->lm_dim;
  const LmArgs g = lm_args(e);
  const size_t cnt = (size_t)n * LM * LM;
  if (cnt == 0) return 0;
  DBuf<uint32_t> d;
  DBuf<double> o;
  if (o.alloc(cnt) != hipSuccess) return e->fail_msg("marginals: output allocation failed");
  hipError_t err = hipSuccess;
  Events<2> ev;
  (void)ev.create();
  if (ids) {
    err = d.alloc(n);
    if (err == hipSuccess) err = hipMemcpy(d.p, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    (void)ev.record(0, e->stream);
    if (err == hipSuccess) {
      if (LM == 1) hipLaunchKernelGGL(k_selinv_lm_ids<1>, dim3((n + 3) / 4), dim3(256), 0, e->stream, g, n, (const uint32_t*)d.p, o.p);
      else hipLaunchKernelGGL(k_selinv_lm_ids<3>, dim3((n + 3) / 4), dim3(256), 0, e->stream, g, n, (const uint32_t*)d.p, o.p);
      err = hipGetLastError();
    }
  } else {
    (void)ev.record(0, e->stream);
    if (st.n_chunks) {
      if (LM == 1) hipLaunchKernelGGL(k_selinv_lm_ranges<1>, dim3((st.n_chunks + 3) / 4), dim3(256), 0, e->stream, g, st.n_chunks, (const uint2*)e->wave_rng.p, o.p);
      else hipLaunchKernelGGL(k_selinv_lm_ranges<3>, dim3((st.n_chunks + 3) / 4), dim3(256), 0, e->stream, g, st.n_chunks, (const uint2*)e->wave_rng.p, o.p);
    }
    if (LM == 1) hipLaunchKernelGGL(k_selinv_lm_bare<1>, dim3((st.L + 3) / 4), dim3(256), 0, e->stream, g, st.L, o.p);
    else hipLaunchKernelGGL(k_selinv_lm_bare<3>, dim3((st.L + 3) / 4), dim3(256), 0, e->stream, g, st.L, o.p);
    err = hipGetLastError();
  }
  (void)ev.record(1, e->stream);
  if (err == hipSuccess) err = hipEventSynchronize(ev[1]);
  if (err == hipSuccess) {
    e->mstats.landmark_ms = ev.ms(0, 1);
    err = hipMemcpy(out, o.p, cnt * sizeof(double), hipMemcpyDeviceToHost);
  }
  return err == hipSuccess ? 0 : e->fail(err, "k_selinv_lm");
}

void marginals_release(Engine* e) {   // (ba_hip_release_marginals promises the memory back while the engine lives)
  e->sig.release(); e->sig_slot.release(); e->sig_col_ptr.release();
  e->sig_col_rows.release(); e->sig_level_cols.release(); e->sig_items.release();
  e->sig_plan = SelinvPlan();
  e->sig_plan_version = ~0ull;
  e->held.selinv_released();
}

}  // namespace bae
