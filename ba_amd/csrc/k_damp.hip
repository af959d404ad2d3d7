// gfx950 kernels of the Levenberg-Marquardt damping (ba_hip_set_damping; the rules are in damping.h, the landmark
// part in k_linearize<.., DAMP = true> of k_proj.hip).  None of them is launched, and no buffer of Engine::damp is
// allocated, unless a linearisation is damped.
//   k_pose_schur_diag   Schur part of every pose's diagonal from its term list       second stream, beside the assembly
//   k_damp_poses        d_p = clamp(S_jj - schur_jj), S_jj += lambda d_p              once A holds the complete S
//   k_damp_terms        pred = delta^T (lambda D delta + g), delta^T D delta, min / max of d     after the back-substitution
//   k_damp_finish       ... their per-wave partials, one wave, in order
#include "engine.h"

namespace bae {

// One workgroup per active pose: sum of a[x] b[x] over the Schur terms (after pose_mid) of its list in pose_ent — the
// diagonal of what k_pose_blocks adds to the pose's block beyond U_ii.  The reduction order of k_pose_blocks: strided
// terms per thread, xor butterfly per wave, waves in order (bitwise reproducible).
__global__ void __launch_bounds__(256)
k_pose_schur_diag(const uint32_t* __restrict__ pose_ptr, const uint32_t* __restrict__ pose_mid,
                  const uint32_t* __restrict__ pose_ent, const double* __restrict__ frow, double* __restrict__ out) {
  __shared__ double red[4][6];
  const uint32_t i = blockIdx.x;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const uint32_t em = pose_mid[i], e1 = pose_ptr[i + 1];
  double acc[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[k] = 0.0;
  for (uint32_t e = em + tid; e < e1; e += 256) {
    const uint32_t ra = pose_ent[3 * (size_t)e], rb = pose_ent[3 * (size_t)e + 1];
    const double2* pa = reinterpret_cast<const double2*>(frow + (size_t)ra * kRow);
    const double2* pb = reinterpret_cast<const double2*>(frow + (size_t)rb * kRow);
    const double2 a0 = pa[0], a1 = pa[1], a2 = pa[2], b0 = pb[0], b1 = pb[1], b2 = pb[2];
    acc[0] += a0.x * b0.x; acc[1] += a0.y * b0.y; acc[2] += a1.x * b1.x;
    acc[3] += a1.y * b1.y; acc[4] += a2.x * b2.x; acc[5] += a2.y * b2.y;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[w][k] = v;
  }
  __syncthreads();
  if (tid < 6) out[(size_t)i * 6 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// One thread per pose parameter j of the np rows of S (engine order).  Unmasked: d_p[j] = clamp(S_jj - schur_jj)
// — U_jj, the pose diagonal of H with the unary, binary, inertial and prior parts that the scatters added to S —
// and S_jj += lambda d_p[j].  Masked: d_p[j] = 0, the 1e6 stays.  Velocity and bias columns have no Schur part.
__global__ void __launch_bounds__(256)
k_damp_poses(uint32_t np, int D, uint32_t ld, double lambda, const uint16_t* __restrict__ mask_opt,
             const double* __restrict__ schur, double* __restrict__ d_p, double* __restrict__ A) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= np) return;
  const uint32_t i = j / (uint32_t)D, k = j - i * (uint32_t)D;
  if (mask_opt[i] & (1u << k)) { d_p[j] = 0.0; return; }
  double* sjj = A + (size_t)j * ld + j;
  const double s = *sjj;
  const double d = damp_pose_diag(s, k < 6 ? schur[(size_t)i * 6 + k] : 0.0);
  d_p[j] = d;
  *sjj = s + lambda * d;
}

// Items: the np pose parameters, then the L landmarks (LM parameters each, the active ones).  Grid-stride over a
// fixed grid, one partial per wave after an xor butterfly: [pred | delta^T D delta | min d | max d][waves].  Masked
// pose parameters (d = 0) and inactive landmarks stay out of the minimum and the maximum.
__global__ void __launch_bounds__(256)
k_damp_terms(uint32_t np, uint32_t L, int LM, double lambda, const int32_t* __restrict__ lm_opt,
             const double* __restrict__ gn_p, const double* __restrict__ rhs_p, const double* __restrict__ d_p,
             const double* __restrict__ gn_l, const double* __restrict__ bl, const double* __restrict__ d_l,
             double* __restrict__ part, uint32_t nwaves) {
  const int lane = threadIdx.x & 63;
  double pred = 0.0, dDd = 0.0, mn = kDampDiagMax, mx = 0.0;
  const size_t total = (size_t)np + L;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    if (idx < np) {
      const double d = d_p[idx];
      damp_term(gn_p[idx], rhs_p[idx], d, lambda, &dDd, &pred);
      if (d > 0.0) { mn = fmin(mn, d); mx = fmax(mx, d); }
    } else {
      const size_t l = idx - np;
      const int lo = lm_opt[l];
      if (lo >= 0)
        for (int k = 0; k < LM; ++k) {
          const double d = d_l[l * LM + k];
          damp_term(gn_l[(size_t)lo * LM + k], bl[l * LM + k], d, lambda, &dDd, &pred);
          if (d > 0.0) { mn = fmin(mn, d); mx = fmax(mx, d); }   // (0: a landmark without observations is never linearised)
        }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    pred += __shfl_xor(pred, off, 64);
    dDd += __shfl_xor(dDd, off, 64);
    mn = fmin(mn, __shfl_xor(mn, off, 64));
    mx = fmax(mx, __shfl_xor(mx, off, 64));
  }
  if (lane == 0) {
    const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
    part[w] = pred; part[(size_t)nwaves + w] = dDd; part[2 * (size_t)nwaves + w] = mn; part[3 * (size_t)nwaves + w] = mx;
  }
}

// one wave: the per-wave partials in order (lane-strided, then the xor butterfly) -> out[0 .. 3]
__global__ void __launch_bounds__(64)
k_damp_finish(uint32_t nwaves, const double* __restrict__ part, double* __restrict__ out) {
  const int lane = threadIdx.x;
  double pred = 0.0, dDd = 0.0, mn = kDampDiagMax, mx = 0.0;
  for (uint32_t w = lane; w < nwaves; w += 64) {
    pred += part[w];
    dDd += part[(size_t)nwaves + w];
    mn = fmin(mn, part[2 * (size_t)nwaves + w]);
    mx = fmax(mx, part[3 * (size_t)nwaves + w]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    pred += __shfl_xor(pred, off, 64);
    dDd += __shfl_xor(dDd, off, 64);
    mn = fmin(mn, __shfl_xor(mn, off, 64));
    mx = fmax(mx, __shfl_xor(mx, off, 64));
  }
  if (lane == 0) { out[0] = pred; out[1] = dDd; out[2] = mn; out[3] = mx; }
}

static uint32_t damp_terms_blocks(const Engine* e) {
  const size_t total = (size_t)e->st.np + e->st.L;
  return (uint32_t)std::min<size_t>(1024, std::max<size_t>((total + 255) / 256, 1));
}

int damp_prepare(Engine* e) {
  if (!(e->damp.lambda_lin > 0.0)) return 0;
  const Structure& st = e->st;
  Engine::Damp& d = e->damp;
  const size_t nl = std::max<size_t>((size_t)st.L * std::max(e->lm_dim, 1), 1);
  BAE_HIP(d.d_p.alloc(std::max<uint32_t>(st.ld, 1)));
  BAE_HIP(d.d_l.alloc(nl));
  BAE_HIP(d.schur.alloc(std::max<size_t>((size_t)st.Pact * 6, 1)));
  BAE_HIP(d.part.alloc((size_t)16 * damp_terms_blocks(e)));
  BAE_HIP(d.out.alloc(4));
  // (inactive landmarks and the padding rows are never written)
  BAE_HIP(hipMemsetAsync(d.d_p.p, 0, d.d_p.bytes(), e->stream));
  BAE_HIP(hipMemsetAsync(d.d_l.p, 0, d.d_l.bytes(), e->stream));
  return 0;
}

int launch_pose_schur_diag(Engine* e) {
  if (!(e->damp.lambda_lin > 0.0) || e->st.Pact == 0) return 0;
  hipLaunchKernelGGL(k_pose_schur_diag, dim3(e->st.Pact), dim3(256), 0, e->stream2, e->pose_ptr.p, e->pose_mid.p,
                     e->pose_ent.p, e->frow.p, e->damp.schur.p);
  BAE_HIP(hipGetLastError());
  return 0;
}

int launch_damp_poses(Engine* e) {
  const Structure& st = e->st;
  if (!(e->damp.lambda_lin > 0.0) || st.np == 0) return 0;
  hipLaunchKernelGGL(k_damp_poses, dim3((st.np + 255) / 256), dim3(256), 0, e->stream, st.np, e->pose_dim, st.ld,
                     e->damp.lambda_lin, (const uint16_t*)(e->pose_mask.p + st.P), (const double*)e->damp.schur.p,
                     e->damp.d_p.p, e->A.p);
  BAE_HIP(hipGetLastError());
  return 0;
}

int launch_damp_terms(Engine* e) {
  const Structure& st = e->st;
  Engine::Damp& d = e->damp;
  if (!(d.lambda_lin > 0.0)) return 0;
  const uint32_t nb = damp_terms_blocks(e), nwaves = 4 * nb;
  hipLaunchKernelGGL(k_damp_terms, dim3(nb), dim3(256), 0, e->stream, st.np, e->lm_dim > 0 && st.Lact > 0 ? st.L : 0u,
                     e->lm_dim, d.lambda_lin, (const int32_t*)e->lm_opt.p, (const double*)e->gn_p.p,
                     (const double*)e->rhs_p.p, (const double*)d.d_p.p, (const double*)e->gn_l.p,
                     (const double*)e->lm_bl.p, (const double*)d.d_l.p, d.part.p, nwaves);
  BAE_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_damp_finish, dim3(1), dim3(64), 0, e->stream, nwaves, (const double*)d.part.p, d.out.p);
  BAE_HIP(hipGetLastError());
  BAE_HIP(hipMemcpyAsync(d.terms_h, d.out.p, sizeof(d.terms_h), hipMemcpyDeviceToHost, e->stream));
  BAE_HIP(hipStreamSynchronize(e->stream));
  d.terms_valid = true;
  return 0;
}

}  // namespace bae
