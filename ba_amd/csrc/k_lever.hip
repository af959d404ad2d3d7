// Leverages of projection residuals (ba_hip_get_projection_leverages): the 2 x 2 diagonal blocks H_aa of the hat
// matrix of the whitened Jacobian, put together from what a direct solve leaves on the device — the factor rows
// (J_m, J_r, W), obs_jl, the calibration rows and the selected inverse Sigma on the factor's tile pattern.
// Formula, listing rule and the host restatement: lever.h; the incidences of a landmark: lm_entry.h.
//
//   k_lever_ranges   every residual: one wavefront per linearisation range (wave_rng), landmark after landmark
//   k_lever_ids      requested residuals: one wavefront per landmark that has any (requests grouped on the host)
//
// Both call lever_landmark, which works a landmark off in batches of 64 observations:
//   rows of t_f = sum_e Sigma_{p_f p_e} W_e, one lane per (incidence f, row i), the sum over e in incidence order,
//   into the wave's LDS stage (64 observation slots + the reference pose's + the calibration's);
//   U = sum_f W_f^T t_f, one lane per slot, summed over the batches per lane, then a fixed butterfly;
//   one lane per observation for the 2 x 2 result.
// A landmark with at most 64 observations has one batch and its t_f stay in the stage.  A longer one does not fit
// (700 incidences x 6 x LM doubles): the sweep over its batches runs twice, first for U alone, then again with
// the 2 x 2 results after each batch that holds a wanted observation — the t_f are recomputed, no global workspace.  No sum depends on the launch
// or on which other residuals were asked for, so a residual's bits are the same from either kernel.  No atomics.
#include "engine.h"
#include "selinv.h"
#include "tile_mma.h"
#include "lm_entry.h"
#include "lever.h"

#include <algorithm>
#include <vector>

namespace bae {

namespace {

struct LevArgs {
  LmArgs g;
  const double* obs_jl;     // [O][2 LM] sqrt(w) dz_dlm (zero for an inactive landmark)
  const double* crow;       // [2 O][6] sqrt(w) dz_dk rows of the observations, or null
  const uint32_t* obs_rid;  // sorted position -> residual id
};

constexpr int kLevBatch = 64;               // observation slots of the stage
constexpr int kLevSlots = kLevBatch + 2;    // + the reference pose's incidence, + the calibration's

// LDS traffic of one wavefront only: order it against the other lanes' accesses
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Rows of t_f for the incidences e0 .. e0 + cnt - 1 of landmark l into the slots s0 .. of the stage:
// stage[(slot * 6 + i) * LM + k] = sum_e sum_j Sigma[f + i][e + j] W_e[k][j]; zero rows for an invalid incidence.
template <int LM>
__device__ __forceinline__ void lever_t_rows(const LmArgs& g, uint32_t l, uint32_t nobs, uint32_t ne, bool any_listed,
                                             uint32_t e0, uint32_t cnt, uint32_t s0, double* __restrict__ stage) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t it = lane; it < cnt * 6; it += 64) {
    const uint32_t s = it / 6, i = it - s * 6;
    const LmEntry<LM> f = lm_entry<LM>(g, l, e0 + s, nobs, any_listed);
    double t[LM];
#pragma unroll
    for (int k = 0; k < LM; ++k) t[k] = 0.0;
    if (f.valid && (int)i < f.width) {
      for (uint32_t e = 0; e < ne; ++e) {
        const LmEntry<LM> x = lm_entry<LM>(g, l, e, nobs, any_listed);
        if (!x.valid) continue;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          if (j < x.width) {
            const double sg = sig_at(g.store, g.slot, g.nt, f.base + i, x.base + j);
#pragma unroll
            for (int k = 0; k < LM; ++k) t[k] += sg * x.w[k * kRow + j];
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < LM; ++k) stage[((s0 + s) * 6 + i) * LM + k] = t[k];
  }
}

// u += W_f^T t_f of the incidence e in slot s
template <int LM>
__device__ __forceinline__ void lever_u_add(const LmArgs& g, uint32_t l, uint32_t nobs, bool any_listed, uint32_t e,
                                            uint32_t s, const double* __restrict__ stage, double (&u)[LM][LM]) {
  const LmEntry<LM> f = lm_entry<LM>(g, l, e, nobs, any_listed);
  if (!f.valid) return;
#pragma unroll
  for (int k1 = 0; k1 < LM; ++k1)
#pragma unroll
    for (int k2 = 0; k2 < LM; ++k2) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i)
        if (i < f.width) acc += f.w[k1 * kRow + i] * stage[(s * 6 + i) * LM + k2];
      u[k1][k2] += acc;
    }
}

// one block of A_a: two rows of `width` values at rows, rows + kRow, against the rows base .. of Sigma; slot: its t_f
struct LevSide {
  bool valid;
  uint32_t base, slot;
  int width;
  const double* rows;
};

// H_aa of observation a (sorted position) of landmark l, t_f of its measuring pose in slot s
template <int LM>
__device__ __forceinline__ void lever_obs(const LevArgs& v, uint32_t l, uint32_t a, uint32_t s, bool act,
                                          const double* __restrict__ stage, const double (&Li)[LM][LM],
                                          const double (&Q)[LM][LM], double* __restrict__ out) {
  constexpr int R = LM == 1 ? 6 : 8;
  const LmArgs& g = v.g;
  const uint32_t pm = g.obs_pose[a], rp = g.lm_ref_pose[l];
  const bool listed = !(LM == 1 && pm == rp);
  const int pom = g.pose_opt[pm], por = g.pose_opt[rp];
  LevSide sd[3];
  sd[0] = {listed && pom >= 0, pom >= 0 ? (uint32_t)pom * g.D : 0, s, 6, g.frow + (size_t)a * R * kRow};
  sd[1] = {LM == 1 && listed && por >= 0, por >= 0 ? (uint32_t)por * g.D : 0, kLevBatch, 6,
           g.frow + ((size_t)a * R + 2) * kRow};
  sd[2] = {g.K > 0 && v.crow != nullptr, g.np, kLevBatch + (LM == 1 ? 1u : 0u), g.K,
           v.crow ? v.crow + 2 * (size_t)a * kRow : nullptr};
  double H[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  // A Sigma A^T over the block pairs (f, g <= f); an off-diagonal pair counts with its transpose
#pragma unroll
  for (int f = 0; f < 3; ++f)
#pragma unroll
    for (int q = 0; q <= f; ++q) {
      if (!sd[f].valid || !sd[q].valid) continue;
      double u0[6], u1[6];  // rows of A_f Sigma_fq
#pragma unroll
      for (int j = 0; j < 6; ++j) u0[j] = u1[j] = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        if (i < sd[f].width) {
          const double a0 = sd[f].rows[i], a1 = sd[f].rows[kRow + i];
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            if (j < sd[q].width) {
              const double sg = sig_at(g.store, g.slot, g.nt, sd[f].base + i, sd[q].base + j);
              u0[j] += a0 * sg;
              u1[j] += a1 * sg;
            }
          }
        }
      }
      double X[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        if (j < sd[q].width) {
          const double b0 = sd[q].rows[j], b1 = sd[q].rows[kRow + j];
          X[0][0] += u0[j] * b0; X[0][1] += u0[j] * b1;
          X[1][0] += u1[j] * b0; X[1][1] += u1[j] * b1;
        }
      }
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) H[r][c] += f == q ? X[r][c] : X[r][c] + X[c][r];
    }
  if (act) {
    double B[2][LM], At[2][LM];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int k = 0; k < LM; ++k) { B[r][k] = v.obs_jl[(size_t)a * 2 * LM + r * LM + k]; At[r][k] = 0.0; }
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      if (!sd[f].valid) continue;
      const double* t = stage + (size_t)sd[f].slot * 6 * LM;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        if (i < sd[f].width) {
#pragma unroll
          for (int k = 0; k < LM; ++k) {
            At[0][k] += sd[f].rows[i] * t[i * LM + k];
            At[1][k] += sd[f].rows[kRow + i] * t[i * LM + k];
          }
        }
      }
    }
    double M[2][LM], N[2][LM], Z[2][LM];  // B Li^T, At Li^T, M Q
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int k2 = 0; k2 < LM; ++k2) {
        double m = 0.0, nn = 0.0;
#pragma unroll
        for (int k = 0; k < LM; ++k) { m += B[r][k] * Li[k2][k]; nn += At[r][k] * Li[k2][k]; }
        M[r][k2] = m; N[r][k2] = nn;
      }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int k2 = 0; k2 < LM; ++k2) {
        double z = 0.0;
#pragma unroll
        for (int k = 0; k < LM; ++k) z += M[r][k] * Q[k][k2];
        Z[r][k2] = z;
      }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        double cr = 0.0, cc = 0.0, p = 0.0;
#pragma unroll
        for (int k = 0; k < LM; ++k) { cr += N[r][k] * M[c][k]; cc += N[c][k] * M[r][k]; p += Z[r][k] * M[c][k]; }
        H[r][c] += p - (cr + cc);
      }
  }
  const double h01 = 0.5 * (H[0][1] + H[1][0]);
  out[0] = H[0][0] + 0.0; out[1] = h01 + 0.0; out[2] = h01 + 0.0; out[3] = H[1][1] + 0.0;
}

// The residuals of landmark l (nobs > 0) by the calling wavefront (all 64 lanes).  nsel == 0: every observation,
// out[4 * residual id]; otherwise the observations at the sorted positions spos[0 .. nsel) alone (ascending, repeats
// allowed), each to out[4 * sq[i]].  The sums of the landmark are formed once, whatever is asked for.
template <int LM>
__device__ void lever_landmark(const LevArgs& v, uint32_t l, const uint32_t* __restrict__ spos,
                               const uint32_t* __restrict__ sq, uint32_t nsel, double* __restrict__ stage,
                               double* __restrict__ out) {
  const LmArgs& g = v.g;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t a0 = g.lm_ptr[l], nobs = g.lm_ptr[l + 1] - a0;
  const bool act = g.lm_opt[l] >= 0;
  bool any_listed = false;
  if (LM == 1) {
    const uint32_t rp = g.lm_ref_pose[l];
    for (uint32_t e0 = 0; e0 < nobs; e0 += 64) {
      const uint32_t e = e0 + lane;
      const bool lst = e < nobs && g.obs_pose[a0 + e] != rp;
      any_listed = any_listed || __ballot(lst) != 0;
    }
  }
  const uint32_t ntail = (LM == 1 ? 1u : 0u) + (g.K > 0 ? 1u : 0u), ne = nobs + ntail;
  const uint32_t nb = (nobs + kLevBatch - 1) / kLevBatch;
  double Li[LM][LM], Q[LM][LM];  // L^-1 of V = L L^T; I + Li U Li^T
#pragma unroll
  for (int a = 0; a < LM; ++a)
#pragma unroll
    for (int b = 0; b < LM; ++b) Li[a][b] = Q[a][b] = 0.0;
  wave_sync();  // the previous landmark's readers are done with the stage
  if (act) {
    double u[LM][LM];
#pragma unroll
    for (int a = 0; a < LM; ++a)
#pragma unroll
      for (int b = 0; b < LM; ++b) u[a][b] = 0.0;
    lever_t_rows<LM>(g, l, nobs, ne, any_listed, nobs, ntail, kLevBatch, stage);
    for (uint32_t b = 0; b < nb; ++b) {
      const uint32_t e0 = b * kLevBatch, cnt = min(nobs - e0, (uint32_t)kLevBatch);
      if (b) wave_sync();
      lever_t_rows<LM>(g, l, nobs, ne, any_listed, e0, cnt, 0, stage);
      wave_sync();
      if (lane < cnt) lever_u_add<LM>(g, l, nobs, any_listed, e0 + lane, lane, stage, u);
      if (b == 0 && lane < ntail) lever_u_add<LM>(g, l, nobs, any_listed, nobs + lane, kLevBatch + lane, stage, u);
    }
#pragma unroll
    for (int a = 0; a < LM; ++a)
#pragma unroll
      for (int b = 0; b < LM; ++b) {
        double x = u[a][b];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
        u[a][b] = x;
      }
    // V = sum_a B_a^T B_a: lane j takes the observations j, j + 64, ..; fixed butterfly
    double V[LM][LM];
#pragma unroll
    for (int a = 0; a < LM; ++a)
#pragma unroll
      for (int b = 0; b < LM; ++b) V[a][b] = 0.0;
    for (uint32_t e = lane; e < nobs; e += 64) {
      const double* B = v.obs_jl + (size_t)(a0 + e) * 2 * LM;
#pragma unroll
      for (int a = 0; a < LM; ++a)
#pragma unroll
        for (int b = 0; b < LM; ++b) V[a][b] += B[a] * B[b] + B[LM + a] * B[LM + b];
    }
#pragma unroll
    for (int a = 0; a < LM; ++a)
#pragma unroll
      for (int b = 0; b < LM; ++b) {
        double x = V[a][b];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
        V[a][b] = x;
      }
    lever_factor<LM>(V, Li);
    double T[LM][LM];  // U Li^T
#pragma unroll
    for (int a = 0; a < LM; ++a)
#pragma unroll
      for (int b = 0; b < LM; ++b) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < LM; ++c) s += u[a][c] * Li[b][c];
        T[a][b] = s;
      }
#pragma unroll
    for (int a = 0; a < LM; ++a)
#pragma unroll
      for (int b = 0; b < LM; ++b) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < LM; ++c) s += Li[a][c] * T[c][b];
        Q[a][b] = (a == b ? 1.0 : 0.0) + s;
      }
  }
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t e0 = b * kLevBatch, cnt = min(nobs - e0, (uint32_t)kLevBatch);
    if (nsel) {  // a batch without a requested observation is skipped (the same answer in every lane)
      bool any = false;
      for (uint32_t i = 0; i < nsel && !any; ++i) any = spos[i] >= a0 + e0 && spos[i] < a0 + e0 + cnt;
      if (!any) continue;
    }
    if (act && nb > 1) {  // the stage holds the last batch of the first sweep
      wave_sync();
      lever_t_rows<LM>(g, l, nobs, ne, any_listed, e0, cnt, 0, stage);
      wave_sync();
    }
    const uint32_t a = a0 + e0 + lane;
    // (one call site of lever_obs: inlined twice, the LmSize 1 kernels went to 256 VGPRs and 152 B of scratch)
    bool want = lane < cnt && !nsel;
    if (lane < cnt)
      for (uint32_t i = 0; i < nsel; ++i) want = want || spos[i] == a;
    if (want) {
      double h[4];
      lever_obs<LM>(v, l, a, lane, act, stage, Li, Q, h);
      if (!nsel) {
        double* o = out + 4 * (size_t)v.obs_rid[a];
        o[0] = h[0]; o[1] = h[1]; o[2] = h[2]; o[3] = h[3];
      } else {
        for (uint32_t i = 0; i < nsel; ++i)
          if (spos[i] == a) {
            double* o = out + 4 * (size_t)sq[i];
            o[0] = h[0]; o[1] = h[1]; o[2] = h[2]; o[3] = h[3];
          }
      }
    }
  }
}

}  // namespace

// every residual: one wavefront per linearisation range; out[4 * residual id]
template <int LM>
__global__ void __launch_bounds__(256) k_lever_ranges(LevArgs v, uint32_t n_rng, const uint2* __restrict__ rng,
                                                      double* __restrict__ out) {
  __shared__ double stage[4][kLevSlots * 6 * LM];
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_rng) return;  // waves are independent: no block-level barrier below
  const uint2 r = rng[q];
  if (r.y <= r.x) return;
  const uint32_t l0 = v.g.obs_lm[r.x], l1 = v.g.obs_lm[r.y - 1];
  for (uint32_t l = l0; l <= l1; ++l)
    if (v.g.lm_ptr[l + 1] > v.g.lm_ptr[l]) lever_landmark<LM>(v, l, nullptr, nullptr, 0, stage[threadIdx.x >> 6], out);
}

// requested residuals: one wavefront per landmark that has any, grp[q] = (first, end) into the requests sorted by
// position (spos: sorted positions, sq: where each goes in out; checked and grouped on the host); out[4 sq[i]]
template <int LM>
__global__ void __launch_bounds__(256) k_lever_ids(LevArgs v, uint32_t n_grp, const uint2* __restrict__ grp,
                                                   const uint32_t* __restrict__ spos, const uint32_t* __restrict__ sq,
                                                   double* __restrict__ out) {
  __shared__ double stage[4][kLevSlots * 6 * LM];
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_grp) return;
  const uint2 r = grp[q];
  lever_landmark<LM>(v, v.g.obs_lm[spos[r.x]], spos + r.x, sq + r.x, r.y - r.x, stage[threadIdx.x >> 6], out);
}

// ---- host side ----------------------------------------------------------------------------------------
// ids: residual ids (checked by the caller), or null for all st.O residuals in residual-id order
int leverages_run(Engine* e, uint32_t n, const uint32_t* ids, double* out) {
  const Structure& st = e->st;
  const int LM = e->lm_dim;
  LevArgs v;
  v.g = lm_args(e);
  v.obs_jl = e->obs_jl.p;
  v.crow = st.K ? e->crow.p : nullptr;
  v.obs_rid = e->obs_rid.p;
  if (n == 0) { e->lstats = {0.0, 0, 0, 0}; return 0; }
  // the plan of the structure, kept until the next ba_hip_finalize: sorted position of every residual id, and
  // the block reads of the all-residuals pass
  if (e->lev_pos.size() != st.O) {
    lever_positions(st.obs_perm, e->lev_pos);
    e->lev_reads_all = lever_block_reads(LM, st.K, st.lm_ptr, st.obs_perm, e->prob.proj_pose, e->prob.proj_lm,
                                         e->prob.lm_ref_pose, st.pose_opt, st.lm_opt, nullptr, st.O, &e->lev_lms_all);
  }
  // requests sorted by position, cut into one group per landmark: [sq | spos | groups (first, end)]
  std::vector<uint32_t> req, spos;
  uint32_t n_grp = 0;
  if (ids) {
    std::vector<uint32_t> ord(n);
    for (uint32_t q = 0; q < n; ++q) ord[q] = q;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return e->lev_pos[ids[x]] < e->lev_pos[ids[y]]; });
    req.resize(2 * (size_t)n);
    spos.resize(n);
    for (uint32_t i = 0; i < n; ++i) { req[i] = ord[i]; req[n + i] = spos[i] = e->lev_pos[ids[ord[i]]]; }
    for (uint32_t i = 0; i < n;) {
      const uint32_t l = e->prob.proj_lm[ids[ord[i]]];
      uint32_t j = i + 1;
      while (j < n && e->prob.proj_lm[ids[ord[j]]] == l) ++j;
      req.push_back(i); req.push_back(j);
      ++n_grp;
      i = j;
    }
  }
  DBuf<uint32_t> d;
  DBuf<double> o;
  if (o.alloc(4 * (size_t)n) != hipSuccess) return e->fail_msg("leverages: output allocation failed");
  hipError_t err = hipSuccess;
  Events<2> ev;
  (void)ev.create();
  const dim3 grid(((ids ? n_grp : st.n_chunks) + 3) / 4), block(256);
  if (ids) {
    err = d.alloc(req.size());
    if (err == hipSuccess) err = hipMemcpy(d.p, req.data(), req.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    (void)ev.record(0, e->stream);
    if (err == hipSuccess) {
      const uint32_t *sq = d.p, *sp = d.p + n;
      const uint2* grp = reinterpret_cast<const uint2*>(d.p + 2 * (size_t)n);
      if (LM == 1) hipLaunchKernelGGL(k_lever_ids<1>, grid, block, 0, e->stream, v, n_grp, grp, sp, sq, o.p);
      else hipLaunchKernelGGL(k_lever_ids<3>, grid, block, 0, e->stream, v, n_grp, grp, sp, sq, o.p);
      err = hipGetLastError();
    }
  } else {
    (void)ev.record(0, e->stream);
    if (LM == 1) hipLaunchKernelGGL(k_lever_ranges<1>, grid, block, 0, e->stream, v, st.n_chunks, (const uint2*)e->wave_rng.p, o.p);
    else hipLaunchKernelGGL(k_lever_ranges<3>, grid, block, 0, e->stream, v, st.n_chunks, (const uint2*)e->wave_rng.p, o.p);
    err = hipGetLastError();
  }
  (void)ev.record(1, e->stream);
  if (err == hipSuccess) err = hipEventSynchronize(ev[1]);
  if (err == hipSuccess) err = hipMemcpy(out, o.p, 4 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
  if (err != hipSuccess) return e->fail(err, "k_lever");
  e->lstats.device_ms = ev.ms(0, 1);
  e->lstats.residuals = n;
  if (ids) {
    e->lstats.block_reads = lever_block_reads(LM, st.K, st.lm_ptr, st.obs_perm, e->prob.proj_pose, e->prob.proj_lm,
                                              e->prob.lm_ref_pose, st.pose_opt, st.lm_opt, spos.data(), n,
                                              &e->lstats.landmarks);
  } else {
    e->lstats.block_reads = e->lev_reads_all;
    e->lstats.landmarks = e->lev_lms_all;
  }
  return 0;
}

}  // namespace bae
