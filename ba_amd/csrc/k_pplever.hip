// Leverages of unary, binary and inertial residuals (ba_hip_get_pose_pose_leverages): per residual the covariance of
// the predicted residual C = J Sigma_ee J^T, the effective information Lambda and the leverage tr(C Lambda), put
// together from what a direct solve leaves on the device — pp_dz, pp_info, the binary weights and square roots,
// and the selected inverse Sigma on the factor's tile pattern.  Formula, the definition of Lambda per kind and the
// host restatement: pplever.h.
//
//   k_pp_lever   one wavefront per requested residual, four per workgroup, all in the wave's LDS stage:
//     Sigma_ee (the D x D blocks of the live poses, through sig_at) and J = [dz1 | dz2] with the columns of masked
//     parameters zeroed and the block of an inactive pose left out (as k_pp_jrhs and k_pp_scatter apply them);
//     T = Sigma_ee J^T; C = J T, one lane per fixed (r, c), sums in index order; C symmetrised; the leverage by a
//     fixed butterfly over the lanes.
// A residual's bits depend on nothing but the residual: not on the launch, not on what else was asked for.
// No atomics, no MFMA (a 15 x 30 x 30 product per wave is no dense contraction worth reshaping).
#include "engine.h"
#include "selinv.h"
#include "tile_mma.h"
#include "lm_entry.h"
#include "pplever.h"

#include <string>
#include <vector>

namespace bae {

namespace {

struct PPLevArgs {
  const uint32_t *res_p1, *res_p2;   // [slots] pose ids, res_p2 = kPPLevNoPose for a unary residual
  const int32_t* pose_opt;
  const uint16_t* pose_mask;         // by pose id
  const double *pp_dz, *pp_info;
  const double *bin_s, *bin_w;       // [binary][36] cov_inv_sqrt, [binary] weight
  const uint32_t* slot;
  const double* store;
  uint32_t nt, slot0;                // tiles per row of the store; first slot of the kind
  int D, R, kind;
};

constexpr int kStageSig = 4 * kPPLevBlock;   // (2 x 15)^2
constexpr int kStageJ = 2 * kPPLevBlock;     // 15 x 30
constexpr int kStage = kStageSig + 2 * kStageJ;

// LDS traffic of one wavefront only: order it against the other lanes' accesses
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

}  // namespace

// cov, info: [n][225], lev: [n], bad: [n] (1: a block of Sigma_ee lies outside the store's pattern);
// ids: ids within the kind, or null for 0 .. n - 1
__global__ void __launch_bounds__(256) k_pp_lever(PPLevArgs v, uint32_t n, const uint32_t* __restrict__ ids,
                                                  double* __restrict__ cov, double* __restrict__ info,
                                                  double* __restrict__ lev, uint32_t* __restrict__ bad) {
  __shared__ double stage[4][kStage];
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n) return;  // waves are independent: no block-level barrier below
  const int lane = threadIdx.x & 63;
  double* sg = stage[threadIdx.x >> 6];   // Sigma_ee (m x m), later C (15 x 15)
  double* J = sg + kStageSig;             // R x m
  double* T = J + kStageJ;                // m x R
  const uint32_t id = ids ? ids[q] : q, slot = v.slot0 + id;
  const int D = v.D, R = v.R, N = kPPLevDim;
  // the live sides, p1 first (at most two: scalars, no indexed private arrays)
  uint32_t b0 = 0, b1 = 0;
  int s0 = 0, s1 = 0, nl = 0;
  uint32_t m0 = 0, m1 = 0;
  for (int s = 0; s < 2; ++s) {
    const uint32_t p = s == 0 ? v.res_p1[slot] : v.res_p2[slot];
    if (p == kPPLevNoPose) continue;
    const int po = v.pose_opt[p];
    if (po < 0) continue;
    if (nl == 0) { b0 = (uint32_t)po * (uint32_t)D; s0 = s; m0 = v.pose_mask[p]; }
    else { b1 = (uint32_t)po * (uint32_t)D; s1 = s; m1 = v.pose_mask[p]; }
    ++nl;
  }
  const int m = nl * D;
  bool nan = false;
  for (int e = lane; e < m * m; e += 64) {
    const int i = e / m, j = e - i * m;
    const uint32_t r = i < D ? b0 + i : b1 + (i - D), c = j < D ? b0 + j : b1 + (j - D);
    const double x = sig_at(v.store, v.slot, v.nt, r, c);
    nan = nan || x != x;
    sg[e] = x;
  }
  const double* dz = v.pp_dz + (size_t)slot * 2 * kPPLevBlock;
  for (int e = lane; e < R * m; e += 64) {
    const int r = e / m, j = e - r * m;
    const bool first = j < D;
    const int c = first ? j : j - D;
    const bool masked = ((first ? m0 : m1) >> c) & 1u;
    J[e] = masked ? 0.0 : dz[(first ? s0 : s1) * kPPLevBlock + r * N + c];
  }
  wave_sync();
  for (int e = lane; e < m * R; e += 64) {   // T = Sigma_ee J^T
    const int i = e / R, r = e - i * R;
    double s = 0.0;
    for (int j = 0; j < m; ++j) s += sg[i * m + j] * J[r * m + j];
    T[e] = s;
  }
  wave_sync();   // every lane is done with Sigma_ee: C takes its place
  for (int e = lane; e < kPPLevBlock; e += 64) {
    const int r = e / N, c = e - r * N;
    double s = 0.0;
    if (r < R && c < R)
      for (int i = 0; i < m; ++i) s += J[r * m + i] * T[i * R + c];
    sg[e] = s;
  }
  wave_sync();
  const double* pinf = v.pp_info + (size_t)slot * kPPLevBlock;
  const double* bs = v.kind == BA_HIP_RES_BINARY ? v.bin_s + (size_t)id * 36 : nullptr;
  const double bw = v.kind == BA_HIP_RES_BINARY ? v.bin_w[id] : 1.0;
  double part = 0.0;
  for (int e = lane; e < kPPLevBlock; e += 64) {
    const int r = e / N, c = e - r * N;
    const bool in = r < R && c < R;
    const double cs = 0.5 * (sg[e] + sg[c * N + r]) + 0.0;
    double l_rc = 0.0, l_cr = 0.0;
    if (in) {
      if (bs) { l_rc = pplever_binary_info(bs, bw, r, c); l_cr = pplever_binary_info(bs, bw, c, r); }
      else { l_rc = pinf[r * N + c]; l_cr = pinf[c * N + r]; }
    }
    part += cs * l_cr;   // tr(C Lambda)
    cov[(size_t)q * kPPLevBlock + e] = cs;
    info[(size_t)q * kPPLevBlock + e] = l_rc;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off, 64);
  const bool any_nan = __ballot(nan) != 0;
  if (lane == 0) { lev[q] = part + 0.0; bad[q] = any_nan ? 1u : 0u; }
}

// ---- host side ----------------------------------------------------------------------------------------
// ids: ids within the kind (checked by the caller), or null for all of the kind in id order; outputs may be null
int pose_pose_leverages_run(Engine* e, int kind, uint32_t n, const uint32_t* ids, double* cov, double* info, double* lev) {
  const Structure& st = e->st;
  const Problem& pb = e->prob;
  e->ppl_stats = {0.0, 0, 0, (uint32_t)kind};
  if (n == 0) return 0;
  PPLevArgs v;
  v.res_p1 = e->pp_res_p1.p; v.res_p2 = e->pp_res_p2.p;
  v.pose_opt = e->pose_opt.p; v.pose_mask = e->lin_pose_mask();   // the masks of the linearisation whose Jacobians pp_dz holds
  v.pp_dz = e->pp_dz.p; v.pp_info = e->pp_info.p;
  v.bin_s = e->bin_cov_inv_sqrt.p; v.bin_w = e->bin_w.p;
  v.slot = e->sig_slot.p; v.store = e->sig.p;
  v.nt = st.ld / TB;
  v.slot0 = kind == BA_HIP_RES_UNARY ? 0u : kind == BA_HIP_RES_BINARY ? pb.num_unary : pb.num_unary + pb.num_binary;
  v.D = e->pose_dim;
  v.R = kind == BA_HIP_RES_IMU ? e->pose_dim : 6;
  v.kind = kind;
  DBuf<uint32_t> d_ids, d_bad;
  DBuf<double> d_out;   // cov | info | leverage
  const size_t nb = (size_t)n * kPPLevBlock;
  if (d_out.alloc(2 * nb + n) != hipSuccess || d_bad.alloc(n) != hipSuccess)
    return e->fail_msg("ba_hip_get_pose_pose_leverages: output allocation failed");
  hipError_t err = hipSuccess;
  if (ids) {
    err = d_ids.alloc(n);
    if (err == hipSuccess) err = hipMemcpy(d_ids.p, ids, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice);
  }
  Events<2> ev;
  (void)ev.create();
  (void)ev.record(0, e->stream);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_pp_lever, dim3((n + 3) / 4), dim3(256), 0, e->stream, v, n, (const uint32_t*)d_ids.p, d_out.p,
                       d_out.p + nb, d_out.p + 2 * nb, d_bad.p);
    err = hipGetLastError();
  }
  (void)ev.record(1, e->stream);
  if (err == hipSuccess) err = hipEventSynchronize(ev[1]);
  std::vector<uint32_t> bad(n);
  if (err == hipSuccess) err = hipMemcpy(bad.data(), d_bad.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (err != hipSuccess) return e->fail(err, "k_pp_lever");
  for (uint32_t q = 0; q < n; ++q)
    if (bad[q])
      return e->fail_msg(("ba_hip_get_pose_pose_leverages: the poses of residual " + std::to_string(ids ? ids[q] : q) +
                          " have a block of Sigma outside the factor's tile pattern").c_str());
  if (cov && err == hipSuccess) err = hipMemcpy(cov, d_out.p, nb * sizeof(double), hipMemcpyDeviceToHost);
  if (info && err == hipSuccess) err = hipMemcpy(info, d_out.p + nb, nb * sizeof(double), hipMemcpyDeviceToHost);
  if (lev && err == hipSuccess) err = hipMemcpy(lev, d_out.p + 2 * nb, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
  if (err != hipSuccess) return e->fail(err, "k_pp_lever");
  const std::vector<uint32_t>& p1 = kind == BA_HIP_RES_UNARY ? pb.un_pose : kind == BA_HIP_RES_BINARY ? pb.bin_p1 : pb.imu_p1;
  const std::vector<uint32_t>& p2 = kind == BA_HIP_RES_BINARY ? pb.bin_p2 : pb.imu_p2;
  uint64_t reads = 0;
  for (uint32_t q = 0; q < n; ++q) {
    const uint32_t id = ids ? ids[q] : q, a = p1[id], b = kind == BA_HIP_RES_UNARY ? kPPLevNoPose : p2[id];
    reads += pplever_block_reads(1, &a, &b, st.pose_opt.data());
  }
  e->ppl_stats.device_ms = ev.ms(0, 1);
  e->ppl_stats.sigma_blocks = reads;
  e->ppl_stats.residuals = n;
  return 0;
}

}  // namespace bae
