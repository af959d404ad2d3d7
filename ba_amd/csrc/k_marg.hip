// Dense pose priors and sliding-window marginalisation.
//
// Consumer — the dense prior residual E_p(x) = c - 2 b^T d + d^T H d on poses p_1 .. p_k (marg.h: d, J_d):
//   k_prior_lin      d and J_d of every covered pose, one lane per pose
//   k_prior_hess     G_ij = J_i^T H_ij J_j, one workgroup per lower D x D block of a prior (mirrored: G is
//                    bitwise symmetric)
//   k_prior_vec      w = b - H d, g = J_d^T w and E_p = c - b^T d - d^T w, one workgroup per prior
//   k_prior_scatter  G and g into A's lower storage, rhs_p and rhs_p_sc; one launch per prior, in prior order,
//                    after k_pp_scatter; one workgroup per block, one thread per element: no atomics
//   k_prior_jrhs     the dogleg term (J_d g)^T H (J_d g), one workgroup per prior
// Producer — ba_hip_marginalize over the local system [M | B] (marg.h: the plan):
//   k_marg_assemble  S^a and rhs^a, one workgroup per lower D x D block, fixed-order term lists
//   k_marg_error     E^a, one lane, fixed order
//   k_marg_ldl       L D L^T of S^a_MM in place, one workgroup (|M| D <= 128)
//   k_marg_trsm      X = L^-1 [S^a_MB | rhs^a_M], one lane per column
//   k_marg_update    H = S^a_BB - X^T D^-1 X, lower triangle, mirrored
//   k_marg_vec       b = rhs^a_B - X^T D^-1 y and c = E^a - y^T D^-1 y
// Every sum runs in a fixed order, so every result is bitwise repeatable.
#include "engine.h"
#include "marg.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace bae {

namespace {

const int kPPH = 225;  // one 15 x 15 block of pp_h

__global__ void k_prior_lin(uint32_t ktot, int D, const uint32_t* __restrict__ pose, const double* __restrict__ x0,
                            const double* __restrict__ state, double* __restrict__ d, double* __restrict__ J) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= ktot) return;
  prior_delta(x0 + (size_t)s * kPoseState, state + (size_t)pose[s] * kPoseState, D, d + (size_t)s * D,
              J ? J + (size_t)s * D * D : nullptr);
}

__global__ void __launch_bounds__(256)
k_prior_hess(int D, const uint2* __restrict__ blk, const uint32_t* __restrict__ ptr,
             const unsigned long long* __restrict__ hoff, const double* __restrict__ H, const double* __restrict__ J,
             double* __restrict__ G) {
  __shared__ double T[kPPH];
  const uint2 bk = blk[blockIdx.x];
  const uint32_t q = bk.x, i = bk.y >> 16, j = bk.y & 0xffffu;
  const uint32_t k0 = ptr[q];
  const size_t kD = (size_t)(ptr[q + 1] - k0) * D;
  const double* Hq = H + hoff[q];
  double* Gq = G + hoff[q];
  const double* Ji = J + (size_t)(k0 + i) * D * D;
  const double* Jj = J + (size_t)(k0 + j) * D * D;
  const int t = threadIdx.x, a = t / D, c = t - a * D;
  const bool elem = t < D * D;
  if (elem) {
    double s = 0.0;
    for (int b = 0; b < D; ++b) s += Hq[((size_t)i * D + a) * kD + (size_t)j * D + b] * Jj[b * D + c];
    T[a * D + c] = s;
  }
  __syncthreads();
  if (elem) {
    const int r = a;
    const int rr = i == j ? max(r, c) : r, cc = i == j ? min(r, c) : c;
    double s = 0.0;
    for (int x = 0; x < D; ++x) s += Ji[x * D + rr] * T[x * D + cc];
    Gq[((size_t)i * D + r) * kD + (size_t)j * D + c] = s;
    if (i != j) Gq[((size_t)j * D + c) * kD + (size_t)i * D + r] = s;
  }
}

// mode 1: w, g and E_p (linearisation); mode 0: w and E_p only (evaluation)
__global__ void __launch_bounds__(256)
k_prior_vec(int D, int mode, const uint32_t* __restrict__ ptr, const unsigned long long* __restrict__ hoff,
            const double* __restrict__ H, const double* __restrict__ b, const double* __restrict__ c,
            const double* __restrict__ d, const double* __restrict__ J, double* __restrict__ w,
            double* __restrict__ g, double* __restrict__ E) {
  const uint32_t q = blockIdx.x, k0 = ptr[q];
  const uint32_t kD = (ptr[q + 1] - k0) * D;
  const double* Hq = H + hoff[q];
  const double* bq = b + (size_t)k0 * D;
  const double* dq = d + (size_t)k0 * D;
  double* wq = w + (size_t)k0 * D;
  for (uint32_t row = threadIdx.x; row < kD; row += blockDim.x) {
    double s = bq[row];
    for (uint32_t col = 0; col < kD; ++col) s -= Hq[(size_t)row * kD + col] * dq[col];
    wq[row] = s;
  }
  __syncthreads();
  if (mode == 1)
    for (uint32_t row = threadIdx.x; row < kD; row += blockDim.x) {
      const uint32_t i = row / D, r = row - i * D;
      const double* Ji = J + (size_t)(k0 + i) * D * D;
      double s = 0.0;
      for (int x = 0; x < D; ++x) s += Ji[x * D + r] * wq[i * D + x];
      g[(size_t)k0 * D + row] = s;
    }
  if (threadIdx.x == 0) {
    double s = c[q];
    for (uint32_t row = 0; row < kD; ++row) s -= bq[row] * dq[row] + dq[row] * wq[row];
    E[q] = s;
  }
}

__global__ void __launch_bounds__(256)
k_prior_scatter(int D, uint32_t ld, const uint2* __restrict__ blk, const uint32_t* __restrict__ ptr,
                const unsigned long long* __restrict__ hoff, const uint32_t* __restrict__ pose,
                const int32_t* __restrict__ pose_opt, const uint16_t* __restrict__ mask, const double* __restrict__ G,
                const double* __restrict__ g, double* __restrict__ A, double* __restrict__ rhs_p,
                double* __restrict__ rhs_sc) {
  const uint2 bk = blk[blockIdx.x];
  const uint32_t q = bk.x, i = bk.y >> 16, j = bk.y & 0xffffu;
  const uint32_t k0 = ptr[q];
  const size_t kD = (size_t)(ptr[q + 1] - k0) * D;
  const uint32_t pi = pose[k0 + i], pj = pose[k0 + j];
  const int32_t oi = pose_opt[pi], oj = pose_opt[pj];
  if (oi < 0 || oj < 0) return;
  const uint16_t mi = mask[pi], mj = mask[pj];
  const int t = threadIdx.x, r = t / D, c = t - r * D;
  if (t < D * D && !(mi & (1u << r)) && !(mj & (1u << c))) {
    const double v = G[hoff[q] + ((size_t)i * D + r) * kD + (size_t)j * D + c];
    if (oi >= oj) A[((size_t)oi * D + r) * ld + (size_t)oj * D + c] += v;
    else A[((size_t)oj * D + c) * ld + (size_t)oi * D + r] += v;
  }
  if (i == j && t < D && !(mi & (1u << t))) {
    const double gv = g[(size_t)(k0 + i) * D + t];
    rhs_p[(size_t)oi * D + t] += gv;
    rhs_sc[(size_t)oi * D + t] += gv;
  }
}

__global__ void __launch_bounds__(256)
k_prior_jrhs(int D, const uint32_t* __restrict__ ptr, const unsigned long long* __restrict__ hoff,
             const uint32_t* __restrict__ pose, const int32_t* __restrict__ pose_opt,
             const uint16_t* __restrict__ mask, const double* __restrict__ H, const double* __restrict__ J,
             const double* __restrict__ rhs_p, double* __restrict__ u, double* __restrict__ out) {
  __shared__ double part[256];
  const uint32_t q = blockIdx.x, k0 = ptr[q];
  const uint32_t kD = (ptr[q + 1] - k0) * D;
  const double* Hq = H + hoff[q];
  double* uq = u + (size_t)k0 * D;
  for (uint32_t row = threadIdx.x; row < kD; row += blockDim.x) {
    const uint32_t i = row / D, r = row - i * D;
    const uint32_t p = pose[k0 + i];
    const int32_t o = pose_opt[p];
    const uint16_t m = mask[p];
    const double* Ji = J + (size_t)(k0 + i) * D * D;
    double s = 0.0;
    if (o >= 0)
      for (int x = 0; x < D; ++x)
        if (!(m & (1u << x))) s += Ji[r * D + x] * rhs_p[(size_t)o * D + x];
    uq[row] = s;
  }
  __syncthreads();
  double acc = 0.0;
  for (uint32_t row = threadIdx.x; row < kD; row += blockDim.x) {
    double s = 0.0;
    for (uint32_t col = 0; col < kD; ++col) s += Hq[(size_t)row * kD + col] * uq[col];
    acc += uq[row] * s;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (unsigned k = 0; k < blockDim.x; ++k) s += part[k];
    out[q] = s;
  }
}

__global__ void k_marg_sum(int n, const double* __restrict__ v, double* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += v[i];
    *out = s;
  }
}

// ---- marginalisation ------------------------------------------------------------------------------
struct MargIn {
  const double *frow, *scal, *pp_h, *pp_g, *pp_err, *G, *g, *E, *lm_vinv;
  const uint32_t* dp_ptr;
  const unsigned long long* hoff;
};

__global__ void __launch_bounds__(256)
k_marg_assemble(int D, uint32_t N, uint32_t nM, const uint32_t* __restrict__ blk_ij, const uint32_t* __restrict__ blk_ptr,
                const uint4* __restrict__ terms, const uint32_t* __restrict__ rhs_ptr, const uint4* __restrict__ rhs_terms,
                const uint16_t* __restrict__ lmask, MargIn in, double* __restrict__ S, double* __restrict__ rhs) {
  const uint32_t bi = blockIdx.x, I = blk_ij[bi] >> 16, J = blk_ij[bi] & 0xffffu;
  const int t = threadIdx.x, r = t / D, c = t - r * D;
  const uint16_t mI = lmask[I], mJ = lmask[J];
  if (t < D * D) {
    const int rr = I == J ? max(r, c) : r, cc = I == J ? min(r, c) : c;
    double s = 0.0;
    for (uint32_t e = blk_ptr[bi]; e < blk_ptr[bi + 1]; ++e) {
      const uint4 tm = terms[e];
      if (tm.x == 0) {
        if (rr < 6 && cc < 6) s += in.frow[(size_t)tm.y * 6 + rr] * in.frow[(size_t)tm.z * 6 + cc];
      } else if (tm.x == 1) {
        const double* h = in.pp_h + (size_t)tm.y * 3 * kPPH;
        const double v = tm.z == 0 ? h[rr * 15 + cc]
                       : tm.z == 1 ? h[kPPH + rr * 15 + cc]
                       : tm.z == 2 ? h[kPPH + cc * 15 + rr] : h[2 * kPPH + rr * 15 + cc];
        s += v;
      } else {
        const size_t kD = (size_t)(in.dp_ptr[tm.y + 1] - in.dp_ptr[tm.y]) * D;
        s += in.G[in.hoff[tm.y] + ((size_t)tm.z * D + rr) * kD + (size_t)tm.w * D + cc];
      }
    }
    // masked parameters: no Jacobian columns; a marginalised one keeps a unit pivot
    if ((mI & (1u << rr)) || (mJ & (1u << cc))) s = (I == J && rr == cc && I < nM) ? 1.0 : 0.0;
    S[((size_t)I * D + r) * N + (size_t)J * D + c] = s;
    if (I != J) S[((size_t)J * D + c) * N + (size_t)I * D + r] = s;
  }
  if (I == J && t < D) {
    double s = 0.0;
    for (uint32_t e = rhs_ptr[I]; e < rhs_ptr[I + 1]; ++e) {
      const uint4 tm = rhs_terms[e];
      if (tm.x == 0) {
        if (t < 6) s += in.frow[(size_t)tm.y * 6 + t] * in.scal[tm.z];
      } else if (tm.x == 1) {
        s += in.pp_g[(size_t)tm.y * 30 + tm.z * 15 + t];
      } else {
        s += in.g[(size_t)(in.dp_ptr[tm.y] + tm.z) * D + t];
      }
    }
    if (mI & (1u << t)) s = 0.0;
    rhs[(size_t)I * D + t] = s;
  }
}

__global__ void k_marg_error(uint32_t n, const uint4* __restrict__ terms, uint32_t O, int LM, MargIn in,
                             double* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s = 0.0;
  for (uint32_t e = 0; e < n; ++e) {
    const uint4 tm = terms[e];
    if (tm.x == 0) {
      const double a = in.scal[2 * (size_t)tm.y], b = in.scal[2 * (size_t)tm.y + 1];
      s += a * a + b * b;
    } else if (tm.x == 1) {
      const double* bl = in.scal + 2 * (size_t)O + (size_t)tm.y * LM;
      const double* Vi = in.lm_vinv + (size_t)tm.y * LM * LM;
      double q = 0.0;
      for (int i = 0; i < LM; ++i)
        for (int j = 0; j < LM; ++j) q += bl[i] * Vi[i * LM + j] * bl[j];
      s -= q;
    } else if (tm.x == 2) {
      s += in.pp_err[tm.y];
    } else {
      s += in.E[tm.y];
    }
  }
  *out = s;
}

// L D L^T of the leading m x m block of S (row stride N) in place: strict lower = L, diagonal = D.
// status = 1 + j for the first pivot with d_j <= tol * S_jj.
__global__ void __launch_bounds__(256)
k_marg_ldl(uint32_t m, uint32_t N, double tol, double* __restrict__ S, int* __restrict__ status) {
  __shared__ double od[kMargMaxM];
  for (uint32_t j = threadIdx.x; j < m; j += blockDim.x) od[j] = S[(size_t)j * N + j];
  __syncthreads();
  int bad = 0;
  for (uint32_t j = 0; j < m; ++j) {
    const double dj = S[(size_t)j * N + j];
    if (!(dj > tol * fabs(od[j])) && bad == 0) bad = 1 + (int)j;
    for (uint32_t i = j + 1 + threadIdx.x; i < m; i += blockDim.x) S[(size_t)i * N + j] /= dj;
    __syncthreads();
    for (uint32_t i = j + 1 + threadIdx.x; i < m; i += blockDim.x) {
      const double lij = S[(size_t)i * N + j] * dj;
      for (uint32_t k = j + 1; k <= i; ++k) S[(size_t)i * N + k] -= lij * S[(size_t)k * N + j];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *status = bad;
}

// columns m .. N of [S | rhs] (column N = rhs): x = L^-1 s over the first m rows, in place
__global__ void k_marg_trsm(uint32_t m, uint32_t N, double* __restrict__ S, double* __restrict__ rhs) {
  const uint32_t col = m + blockIdx.x * blockDim.x + threadIdx.x;
  if (col > N) return;
  for (uint32_t i = 0; i < m; ++i) {
    double s = col < N ? S[(size_t)i * N + col] : rhs[i];
    for (uint32_t k = 0; k < i; ++k) s -= S[(size_t)i * N + k] * (col < N ? S[(size_t)k * N + col] : rhs[k]);
    if (col < N) S[(size_t)i * N + col] = s;
    else rhs[i] = s;
  }
}

// H = S_BB - X^T D^-1 X on 64 x 64 tiles of the lower triangle; element (i, j), i >= j, mirrored
__global__ void __launch_bounds__(256)
k_marg_update(uint32_t m, uint32_t N, const double* __restrict__ S, double* __restrict__ H) {
  const uint32_t nb = N - m;
  // tile index -> (ti, tj), tj <= ti
  const uint32_t t = blockIdx.x;
  uint32_t ti = (uint32_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  while (ti * (ti + 1) / 2 > t) --ti;
  const uint32_t tj = t - ti * (ti + 1) / 2;
  for (uint32_t e = threadIdx.x; e < 64 * 64; e += blockDim.x) {
    const uint32_t i = ti * 64 + e / 64, j = tj * 64 + (e & 63);
    if (i >= nb || j > i) continue;
    double s = S[(size_t)(m + i) * N + m + j];
    for (uint32_t k = 0; k < m; ++k)
      s -= (S[(size_t)k * N + m + i] / S[(size_t)k * N + k]) * S[(size_t)k * N + m + j];
    H[(size_t)i * nb + j] = s;
    H[(size_t)j * nb + i] = s;
  }
}

// b_i = rhs_B[i] - sum_k X[k][i] y_k / d_k (i < nb); c = E^a - sum_k y_k^2 / d_k (i == nb)
__global__ void k_marg_vec(uint32_t m, uint32_t N, const double* __restrict__ S, const double* __restrict__ rhs,
                           const double* __restrict__ Ea, double* __restrict__ b, double* __restrict__ c) {
  const uint32_t nb = N - m;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nb) return;
  double s = i < nb ? rhs[m + i] : *Ea;
  for (uint32_t k = 0; k < m; ++k) {
    const double yk = rhs[k] / S[(size_t)k * N + k];
    s -= (i < nb ? S[(size_t)k * N + m + i] : rhs[k]) * yk;
  }
  if (i < nb) b[i] = s;
  else *c = s;
}

// a fixed-order sum of n device doubles into *host (deferred while the engine defers its sums)
int small_sum(Engine* e, int n, const double* d_v, double* host) {
  *host = 0.0;
  if (n <= 0) return 0;
  if (e->defer_active && e->defer_n < 40) {
    hipLaunchKernelGGL(k_marg_sum, dim3(1), dim3(1), 0, e->stream, n, d_v, e->scalars_out.p + 16 + e->defer_n);
    BAE_HIP(hipGetLastError());
    e->defer_host[e->defer_n++] = host;
    return 0;
  }
  hipLaunchKernelGGL(k_marg_sum, dim3(1), dim3(1), 0, e->stream, n, d_v, e->scalars_out.p + 8);
  BAE_HIP(hipGetLastError());
  BAE_HIP(hipMemcpyAsync(host, e->scalars_out.p + 8, sizeof(double), hipMemcpyDeviceToHost, e->stream));
  BAE_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

}  // namespace

// ---- dense priors ---------------------------------------------------------------------------------
int priors_upload(Engine* e) {
  DensePriors& pr = e->dpri;
  const int D = e->pose_dim;
  const uint32_t nq = pr.count();
  e->dp_blk_first.assign(nq + 1, 0);
  e->dp_E_last = nullptr;
  if (nq == 0) return 0;
  if (e->calib_dim) return e->fail_msg("dense priors are not offered with calibration unknowns");
  const Problem& pb = e->prob;
  for (uint32_t q = 0; q < nq; ++q)
    for (uint32_t k = pr.ptr[q]; k < pr.ptr[q + 1]; ++k) {
      if (pr.pose[k] >= pb.num_poses) return e->fail_msg("dense prior on an unknown pose");
      for (uint32_t k2 = pr.ptr[q]; k2 < k; ++k2)
        if (pr.pose[k2] == pr.pose[k]) return e->fail_msg("dense prior lists a pose twice");
    }
  pr.offsets(D);
  std::vector<uint2> blk;
  std::vector<unsigned long long> hoff(pr.h_off.begin(), pr.h_off.end());
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t k = pr.ptr[q + 1] - pr.ptr[q];
    for (uint32_t i = 0; i < k; ++i)
      for (uint32_t j = 0; j <= i; ++j) blk.push_back(make_uint2(q, i << 16 | j));
    e->dp_blk_first[q + 1] = (uint32_t)blk.size();
  }
  const size_t ktot = pr.pose.size();
  int rc;
  if ((rc = upload_async(e, e->dp_ptr, pr.ptr.data(), pr.ptr.size())) ||
      (rc = upload_async(e, e->dp_pose, pr.pose.data(), ktot)) ||
      (rc = upload_async(e, e->dp_x0, pr.x0.data(), pr.x0.size())) ||
      (rc = upload_async(e, e->dp_H, pr.H.data(), pr.H.size())) ||
      (rc = upload_async(e, e->dp_b, pr.b.data(), pr.b.size())) ||
      (rc = upload_async(e, e->dp_c, pr.c.data(), pr.c.size())) ||
      (rc = upload_async(e, e->dp_hoff, hoff.data(), hoff.size())) ||
      (rc = upload_async(e, e->dp_blk, blk.data(), blk.size())))
    return rc;
  BAE_HIP(e->dp_d.alloc(ktot * D)); BAE_HIP(e->dp_J.alloc(ktot * D * D));
  BAE_HIP(e->dp_G.alloc(std::max<size_t>(pr.h_off[nq], 1))); BAE_HIP(e->dp_g.alloc(ktot * D));
  BAE_HIP(e->dp_w.alloc(ktot * D));
  BAE_HIP(e->dp_E.alloc(nq)); BAE_HIP(e->dp_E_eval.alloc(nq)); BAE_HIP(e->dp_jr.alloc(nq));
  BAE_HIP(hipMemsetAsync(e->dp_E.p, 0, e->dp_E.bytes(), e->stream));
  BAE_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

// linearisation (mode 1) or evaluation (mode 0) of every prior at the current state; E_p summed into *err_host
int launch_priors(Engine* e, int mode, double* err_host) {
  *err_host = 0.0;
  const uint32_t nq = e->dpri.count();
  if (nq == 0) return 0;
  if (e->sharded()) return e->fail_msg("dense priors are not offered on sharded engines");
  const int D = e->pose_dim;
  const uint32_t ktot = (uint32_t)e->dpri.pose.size();
  const double* state = e->pose_state[e->cur].p;
  double* E = mode ? e->dp_E.p : e->dp_E_eval.p;
  hipLaunchKernelGGL(k_prior_lin, dim3((ktot + 63) / 64), dim3(64), 0, e->stream, ktot, D, e->dp_pose.p, e->dp_x0.p,
                     state, e->dp_d.p, mode ? e->dp_J.p : (double*)nullptr);
  BAE_HIP(hipGetLastError());
  if (mode) {
    hipLaunchKernelGGL(k_prior_hess, dim3(e->dp_blk_first[nq]), dim3(256), 0, e->stream, D,
                       (const uint2*)e->dp_blk.p, e->dp_ptr.p, e->dp_hoff.p, e->dp_H.p, e->dp_J.p, e->dp_G.p);
    BAE_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_prior_vec, dim3(nq), dim3(256), 0, e->stream, D, mode, e->dp_ptr.p, e->dp_hoff.p, e->dp_H.p,
                     e->dp_b.p, e->dp_c.p, e->dp_d.p, e->dp_J.p, e->dp_w.p, e->dp_g.p, E);
  BAE_HIP(hipGetLastError());
  if (mode)
    for (uint32_t q = 0; q < nq; ++q) {  // in prior order, after k_pp_scatter
      const uint32_t b0 = e->dp_blk_first[q], nb = e->dp_blk_first[q + 1] - b0;
      hipLaunchKernelGGL(k_prior_scatter, dim3(nb), dim3(256), 0, e->stream, D, e->st.ld,
                         (const uint2*)e->dp_blk.p + b0, e->dp_ptr.p, e->dp_hoff.p, e->dp_pose.p, e->pose_opt.p,
                         e->pose_mask.p, e->dp_G.p, e->dp_g.p, e->A.p, e->rhs_p.p, e->rhs_sc.p);
      BAE_HIP(hipGetLastError());
    }
  e->dp_E_last = E;
  return small_sum(e, (int)nq, E, err_host);
}

int launch_priors_jrhs(Engine* e, double* out) {
  *out = 0.0;
  const uint32_t nq = e->dpri.count();
  if (nq == 0) return 0;
  hipLaunchKernelGGL(k_prior_jrhs, dim3(nq), dim3(256), 0, e->stream, e->pose_dim, e->dp_ptr.p, e->dp_hoff.p,
                     e->dp_pose.p, e->pose_opt.p, e->pose_mask.p, e->dp_H.p, e->dp_J.p, e->rhs_p.p, e->dp_w.p,
                     e->dp_jr.p);
  BAE_HIP(hipGetLastError());
  return small_sum(e, (int)nq, e->dp_jr.p, out);
}

// ---- marginalisation ------------------------------------------------------------------------------
int marginalize_run(Engine* e, const MargPlan& pl, const std::vector<uint16_t>& lmask, double tol, double* dev_ms) {
  const int D = e->pose_dim;
  const uint32_t n = pl.nM + pl.nB, N = n * D, m = pl.nM * D, nb = pl.nB * D;
  static_assert(sizeof(MargTerm) == sizeof(uint4), "term records are plain words");
  DBuf<uint32_t> blk_ij, blk_ptr, rhs_ptr;
  DBuf<uint4> terms, rterms, eterms;
  DBuf<uint16_t> dmask;
  DBuf<double> S, rhs, Ea, Hd, bd;
  DBuf<int32_t> status;
  Events<2> ev;
  int rc;
  if ((rc = upload_async(e, blk_ij, pl.blk_ij.data(), pl.blk_ij.size())) ||
      (rc = upload_async(e, blk_ptr, pl.blk_ptr.data(), pl.blk_ptr.size())) ||
      (rc = upload_async(e, terms, pl.blk_terms.data(), pl.blk_terms.size())) ||
      (rc = upload_async(e, rhs_ptr, pl.rhs_ptr.data(), pl.rhs_ptr.size())) ||
      (rc = upload_async(e, rterms, pl.rhs_terms.data(), pl.rhs_terms.size())) ||
      (rc = upload_async(e, eterms, pl.err_terms.data(), pl.err_terms.size())) ||
      (rc = upload_async(e, dmask, lmask.data(), lmask.size())))
    return rc;
  BAE_HIP(S.alloc((size_t)N * N)); BAE_HIP(rhs.alloc(N)); BAE_HIP(Ea.alloc(1));
  BAE_HIP(Hd.alloc(std::max<size_t>((size_t)nb * nb, 1))); BAE_HIP(bd.alloc(nb + 1)); BAE_HIP(status.alloc(1));
  BAE_HIP(hipMemsetAsync(S.p, 0, S.bytes(), e->stream));
  BAE_HIP(ev.create());
  BAE_HIP(ev.record(0, e->stream));
  MargIn in;
  in.frow = e->frow.p; in.scal = e->scal.p; in.pp_h = e->pp_h.p; in.pp_g = e->pp_g.p; in.pp_err = e->pp_err_lin.p;
  in.G = e->dp_G.p; in.g = e->dp_g.p; in.E = e->dp_E.p; in.lm_vinv = e->lm_vinv.p;
  in.dp_ptr = e->dp_ptr.p; in.hoff = e->dp_hoff.p;
  hipLaunchKernelGGL(k_marg_assemble, dim3((uint32_t)pl.blk_ij.size()), dim3(256), 0, e->stream, D, N, pl.nM,
                     blk_ij.p, blk_ptr.p, terms.p, rhs_ptr.p, rterms.p, dmask.p, in, S.p, rhs.p);
  BAE_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_marg_error, dim3(1), dim3(1), 0, e->stream, (uint32_t)pl.err_terms.size(), eterms.p, e->st.O,
                     e->lm_dim, in, Ea.p);
  BAE_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_marg_ldl, dim3(1), dim3(256), 0, e->stream, m, N, tol, S.p, status.p);
  BAE_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_marg_trsm, dim3((nb + 1 + 63) / 64), dim3(64), 0, e->stream, m, N, S.p, rhs.p);
  BAE_HIP(hipGetLastError());
  const uint32_t nt = (nb + 63) / 64;
  if (nt) {
    hipLaunchKernelGGL(k_marg_update, dim3(nt * (nt + 1) / 2), dim3(256), 0, e->stream, m, N, S.p, Hd.p);
    BAE_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_marg_vec, dim3((nb + 1 + 63) / 64), dim3(64), 0, e->stream, m, N, S.p, rhs.p, Ea.p, bd.p,
                     bd.p + nb);
  BAE_HIP(hipGetLastError());
  int32_t st_h = 0;
  e->marg_H.assign((size_t)nb * nb, 0.0);
  e->marg_b.assign(nb + 1, 0.0);
  BAE_HIP(hipMemcpyAsync(&st_h, status.p, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  if (nb) BAE_HIP(hipMemcpyAsync(e->marg_H.data(), Hd.p, (size_t)nb * nb * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  BAE_HIP(hipMemcpyAsync(e->marg_b.data(), bd.p, (nb + 1) * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  BAE_HIP(ev.record(1, e->stream));
  BAE_HIP(hipStreamSynchronize(e->stream));
  *dev_ms = ev.ms(0, 1);
  e->marg_c = e->marg_b[nb];
  e->marg_b.resize(nb);
  if (st_h) {
    e->err = "marginalize: S^a_MM is not positive definite (pivot " + std::to_string(st_h - 1) +
             "): the absorbed residuals do not determine M";
    return BA_HIP_FACTORIZATION_ERROR;
  }
  return 0;
}

}  // namespace bae
