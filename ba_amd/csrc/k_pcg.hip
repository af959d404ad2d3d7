// Block-Jacobi preconditioned conjugate gradients on the reduced camera system (pcg.h has the algorithm, the
// plan and the host restatement).  One pass is four launches: k_pcg_spmv_tiles, k_pcg_spmv_gather, k_pcg_update1,
// k_pcg_update2 (six with the two-level preconditioner: the two coarse launches of k_pcg_coarse.hip run between
// update1 and update2<true>, which adds the prolongated coarse correction to z); every kernel starts by reading the device state and returns at once when `done` is set, so the
// host enqueues check_every passes blind and reads the state back once per batch.  FP64 VALU only (a mat-vec has no
// use for MFMA), no atomics, every sum in a fixed order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "engine.h"

namespace bae {

// sum of n partials by one block of 256 threads, the same value in every block (pcg_block_sum)
static __device__ __forceinline__ double block_sum256(const double* __restrict__ parts, uint32_t n, double* red) {
  double s = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += 256) s += parts[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const double v = red[0];
  __syncthreads();
  return v;
}

// One workgroup per tile (I, J) of the plan: the 32 KB tile is read once, 16 bytes per lane (a wavefront covers
// two rows of 64 doubles per load, the eight loads of a lane are independent).  Lane (rg, c2) owns the columns
// 2 c2, 2 c2 + 1 of the rows rg + 8 k.  Row sums A v_J and column sums A^T v_I go through LDS and are summed in a
// fixed order into the tile's two slots.  Diagonal tiles: lower triangle only (see pcg.h).
__global__ __launch_bounds__(256) void k_pcg_spmv_tiles(const double* __restrict__ A, uint32_t ld,
                                                        const uint2* __restrict__ tiles, const double* __restrict__ p,
                                                        const double* __restrict__ x, const PcgState* __restrict__ st,
                                                        double* __restrict__ rowslot, double* __restrict__ colslot) {
  if (st->done) return;
  const double* v = st->mode == kPcgVerify ? x : p;
  __shared__ double vI[64], vJ[64];
  __shared__ double rpart[64][33];
  __shared__ double cpart[8][64];
  const uint32_t tid = threadIdx.x, c2 = tid & 31u, rg = tid >> 5;
  const uint2 t = tiles[blockIdx.x];
  const uint32_t I = t.x, J = t.y;
  const bool diag = I == J;
  const double* base = A + (size_t)I * 64 * ld + (size_t)J * 64 + 2 * c2;
  double2 a[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = *reinterpret_cast<const double2*>(base + (size_t)(rg + 8 * k) * ld);
  if (tid < 64) vI[tid] = v[(size_t)I * 64 + tid];
  else if (tid < 128) vJ[tid - 64] = v[(size_t)J * 64 + tid - 64];
  __syncthreads();
  const double vj0 = vJ[2 * c2], vj1 = vJ[2 * c2 + 1];
  const uint32_t c = 2 * c2;
  double s0 = 0.0, s1 = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t r = rg + 8 * k;
    const double a0 = diag && c > r ? 0.0 : a[k].x;
    const double a1 = diag && c + 1 > r ? 0.0 : a[k].y;
    rpart[r][c2] = a0 * vj0 + a1 * vj1;
    const double vi = vI[r];
    s0 += (diag && c >= r ? 0.0 : a[k].x) * vi;
    s1 += (diag && c + 1 >= r ? 0.0 : a[k].y) * vi;
  }
  cpart[rg][c] = s0;
  cpart[rg][c + 1] = s1;
  __syncthreads();
  if (tid < 64) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 32; ++j) s += rpart[tid][j];
    rowslot[(size_t)blockIdx.x * 64 + tid] = s;
  } else if (tid < 128) {
    const uint32_t cc = tid - 64;
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < 8; ++g) s += cpart[g][cc];
    colslot[(size_t)blockIdx.x * 64 + cc] = s;
  }
}

// One wavefront per tile row I: q_I = row slots of tile row I (ascending J) + column slots of tile column I
// (ascending row); the partial sum of p.q of these 64 rows.
__global__ __launch_bounds__(64) void k_pcg_spmv_gather(const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col_ptr,
                                                        const uint32_t* __restrict__ col_slot, const double* __restrict__ rowslot,
                                                        const double* __restrict__ colslot, const double* __restrict__ p,
                                                        const PcgState* __restrict__ st, double* __restrict__ q,
                                                        double* __restrict__ pq_part) {
  if (st->done) return;
  __shared__ double red[64];
  const uint32_t I = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  for (uint32_t e = row_ptr[I]; e < row_ptr[I + 1]; ++e) s += rowslot[(size_t)e * 64 + t];
  for (uint32_t e = col_ptr[I]; e < col_ptr[I + 1]; ++e) s += colslot[(size_t)col_slot[e] * 64 + t];
  q[(size_t)I * 64 + t] = s;
  red[t] = p[(size_t)I * 64 + t] * s;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if ((int)t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) pq_part[I] = red[0];
}

// Preconditioner: four blocks per wavefront, 16 lanes each, lane j owns column j of its block in LDS
// (pcg_invert_block).  Elements of tiles outside the pattern count as zero; a pivot that is not positive and
// finite sets *status.
__global__ __launch_bounds__(64) void k_pcg_blocks(const double* __restrict__ A, uint32_t ld, const uint8_t* __restrict__ nz,
                                                   uint32_t nt, const uint2* __restrict__ blocks, uint32_t nblocks,
                                                   double* __restrict__ minv, int32_t* __restrict__ status) {
  __shared__ double a[4][16][17];
  const uint32_t g = threadIdx.x >> 4, l = threadIdx.x & 15u;
  const uint32_t b = blockIdx.x * 4 + g;
  const bool valid = b < nblocks;
  const uint2 bs = valid ? blocks[b] : make_uint2(0, 0);
  const uint32_t start = bs.x, D = bs.y;
  const bool lane_on = valid && l < D;
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) {
    double v = 0.0;
    if (lane_on && i < D) {
      const uint32_t r = start + (i > l ? i : l), c = start + (i > l ? l : i);
      if (r / 64 == c / 64 || nz[(size_t)(r / 64) * nt + c / 64]) v = A[(size_t)r * ld + c];
    }
    a[g][i][l] = v;
  }
  bool ok = true;
  for (uint32_t k = 0; k < kPcgMaxBlock; ++k) {
    __syncthreads();
    const double piv = a[g][k][k];
    const bool good = piv > 0.0 && pcg_finite(piv);
    if (valid && k < D && !good) ok = false;
    const double ip = good ? 1.0 / piv : 0.0;
    double f[16];
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) f[i] = a[g][i][k];
    const double akl = a[g][k][l];
    __syncthreads();
    if (lane_on && k < D) {
      const double rk = l == k ? ip : akl * ip;
#pragma unroll
      for (uint32_t i = 0; i < 16; ++i)
        if (i < D && i != k) a[g][i][l] = l == k ? -f[i] * ip : a[g][i][l] - f[i] * rk;
      a[g][k][l] = rk;
    }
  }
  __syncthreads();
  if (lane_on) {
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
      if (i < D) minv[(size_t)(start + i) * 16 + l] = 0.5 * (a[g][i][l] + a[g][l][i]);
    if (!ok) *status = 1;
  }
}

// r = r - alpha q (kPcgIter: alpha from the fixed-order sum of p.q), r = rhs (kPcgInit) or r = rhs - q (kPcgVerify);
// z = M^-1 r, one thread per row over the rows of its block; partial sums of r.z and r.r per block of 256 rows.
__global__ __launch_bounds__(256) void k_pcg_update1(uint32_t n, uint32_t ld, uint32_t nt, const PcgState* __restrict__ st,
                                                     const double* __restrict__ pq_part, const double* __restrict__ rhs,
                                                     const double* __restrict__ q, const double* __restrict__ r_in,
                                                     const uint2* __restrict__ blk, const double* __restrict__ minv,
                                                     double* __restrict__ r_out, double* __restrict__ z,
                                                     double* __restrict__ rz_part, double* __restrict__ rr_part) {
  __shared__ double red[256];
  __shared__ double red2[256];
  const PcgState s = *st;
  if (s.done) return;
  double alpha = 0.0;
  if (s.mode == kPcgIter) {
    const double pq = block_sum256(pq_part, nt, red);
    alpha = s.rz_old / pq;
    if (!(pcg_finite(pq) && pq > 0.0 && pcg_finite(alpha))) return;   // the same in every block: update2 reports it
  }
  const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
  double rn = 0.0, zz = 0.0;
  if (row < n) {
    const uint2 b = blk[row];
    for (uint32_t j = 0; j < b.y; ++j) {
      const size_t c = b.x + j;
      const double rj = s.mode == kPcgIter ? r_in[c] - alpha * q[c] : s.mode == kPcgInit ? rhs[c] : rhs[c] - q[c];
      if (c == row) rn = rj;
      zz += minv[row * 16 + j] * rj;
    }
  }
  if (row < ld) { r_out[row] = rn; z[row] = zz; }
  red[threadIdx.x] = rn * zz;
  red2[threadIdx.x] = rn * rn;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { red[threadIdx.x] += red[threadIdx.x + w]; red2[threadIdx.x] += red2[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { rz_part[blockIdx.x] = red[0]; rr_part[blockIdx.x] = red2[0]; }
}

// Sums the partials (every block forms the same three scalars), decides (pcg_decide), moves x and p; block 0
// writes the next state into the other copy.  COARSE: z = z_bj + y_c[cmap[row]] and r.z = r.z_bj + r_c.y_c (the sum
// of the nc partials of k_pcg_coarse_apply); the coarse factorisation's status word is bit 1 of the block status.
template <bool COARSE>
__global__ __launch_bounds__(256) void k_pcg_update2(uint32_t ld, uint32_t nt, uint32_t nb, const PcgState* __restrict__ st,
                                                     PcgState* __restrict__ st_out, const int32_t* __restrict__ status,
                                                     const double* __restrict__ pq_part, const double* __restrict__ rz_part,
                                                     const double* __restrict__ rr_part, const double* __restrict__ z,
                                                     double* __restrict__ x, double* __restrict__ p, uint32_t nc,
                                                     const uint32_t* __restrict__ cmap, const double* __restrict__ yc,
                                                     const double* __restrict__ ryc_part) {
  __shared__ double red[256];
  const PcgState s = *st;
  if (s.done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *st_out = s;
    return;
  }
  const double pq = s.mode == kPcgIter ? block_sum256(pq_part, nt, red) : 0.0;
  double rz = block_sum256(rz_part, nb, red);
  const double rr = block_sum256(rr_part, nb, red);
  int block_status = status[0];
  if (COARSE) {
    rz += block_sum256(ryc_part, nc, red);
    block_status = (status[0] ? 1 : 0) | (status[1] ? 2 : 0);
  }
  PcgState o;
  double alpha, beta;
  const uint32_t act = pcg_decide(s, pq, rz, rr, block_status, o, alpha, beta);
  const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (row < ld) {
    const double pv = p[row];
    double zr = z[row];
    if (COARSE) {
      const uint32_t c = cmap[row];
      if (c != kPcgNone) zr += yc[c];
    }
    if (act & kPcgStep) x[row] += alpha * pv;
    if (act & kPcgDir) p[row] = zr + beta * pv;
    else if (act & kPcgRestart) p[row] = zr;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *st_out = o;
}

int pcg_solve_device(Engine* e, const double* dA, uint32_t n, uint32_t ld, const double* d_rhs, const PcgPlan& plan,
                     const std::vector<uint8_t>& nz, const std::vector<uint32_t>& blk, const std::vector<uint32_t>& blocks,
                     bool upload, const ba_hip_pcg_options& opt, double* dx, ba_hip_pcg_stats* stats, int* status) {
  Engine::PcgWork& w = e->pcg;
  hipStream_t s = e->stream;
  const uint32_t nt = plan.nt, nb = (ld + 255) / 256, nblocks = (uint32_t)(blocks.size() / 2);
  int rc;
  memset(stats, 0, sizeof(*stats));
  *status = 0;
  if (ld != 64 * nt || blk.size() != (size_t)2 * ld || nz.size() != (size_t)nt * nt)
    return e->fail_msg("pcg_solve_device: plan does not match the system");
  e->held.pcg_run_begins();
  const bool coarse = opt.coarse_aggregate != 0;
  if (coarse && (plan.cmap.size() != (size_t)ld || plan.coarse_req != opt.coarse_aggregate || plan.ncp % 64 || plan.nc > plan.ncp))
    return e->fail_msg("pcg_solve_device: the plan's coarse space does not match the options");
  // event pairs: 0 / 5 the solve, 1 / 2 the block inverses, 3 / 4 one mat-vec of a batch, 6 / 7 the coarse setup,
  // 8 / 9 one coarse apply of a batch
  Events<10> ev;
  BAE_HIP(ev.create());
  BAE_HIP(ev.record(0, s));
  if (upload || !w.tiles.p) {
    if ((rc = upload_async(e, w.tiles, plan.tiles.data(), plan.tiles.size())) ||
        (rc = upload_async(e, w.blk, blk.data(), blk.size())) ||
        (rc = upload_async(e, w.blocks, blocks.data(), blocks.size())) ||
        (rc = upload_async(e, w.row_ptr, plan.row_ptr.data(), plan.row_ptr.size())) ||
        (rc = upload_async(e, w.col_ptr, plan.col_ptr.data(), plan.col_ptr.size())) ||
        (rc = upload_async(e, w.col_slot, plan.col_slot.data(), plan.col_slot.size())) ||
        (rc = upload_async(e, w.nz, nz.data(), nz.size())))
      return rc;
    BAE_HIP(w.rowslot.alloc((size_t)plan.n_tiles * 64));
    BAE_HIP(w.colslot.alloc((size_t)plan.n_tiles * 64));
    BAE_HIP(w.minv.alloc((size_t)ld * 16));
    BAE_HIP(w.x.alloc(ld)); BAE_HIP(w.r.alloc((size_t)2 * ld)); BAE_HIP(w.z.alloc(ld)); BAE_HIP(w.p.alloc(ld)); BAE_HIP(w.q.alloc(ld));
    BAE_HIP(w.parts.alloc((size_t)nt + 2 * nb));
    BAE_HIP(w.state.alloc(2));
    BAE_HIP(w.status.alloc(2));
  }
  const uint32_t nc = plan.nc, ncp = plan.ncp;
  if (upload) w.coarse_key = 0;   // the work space changes hands: coarse tables uploaded earlier belong to another system
  if (coarse) {
    if (upload || w.coarse_key != plan.coarse_req || !w.cmap.p) {
      if ((rc = upload_async(e, w.cmap, plan.cmap.data(), plan.cmap.size())) ||
          (rc = upload_async(e, w.crow_ptr, plan.crow_ptr.data(), plan.crow_ptr.size())) ||
          (rc = upload_async(e, w.crow_rows, plan.crow_rows.data(), plan.crow_rows.size())))
        return rc;
      w.coarse_key = plan.coarse_req;
    }
    BAE_HIP(w.C.alloc((size_t)ncp * ncp)); BAE_HIP(w.Lc.alloc((size_t)ncp * ncp)); BAE_HIP(w.Wc.alloc((size_t)ncp * ncp));
    BAE_HIP(w.Cinv.alloc((size_t)ncp * ncp));
    BAE_HIP(w.rc.alloc(ncp)); BAE_HIP(w.yc.alloc(ncp)); BAE_HIP(w.ryc_part.alloc(ncp));
  }
  w.coarse_nc = w.coarse_ncp = 0;
  double* pq_part = w.parts.p;
  double* rz_part = w.parts.p + nt;
  double* rr_part = rz_part + nb;
  PcgState h0;
  memset(&h0, 0, sizeof(h0));
  h0.tol2 = opt.rel_tolerance * opt.rel_tolerance;
  h0.max_it = opt.max_iterations ? opt.max_iterations : n;
  h0.mode = kPcgInit;
  const uint32_t check_every = opt.check_every ? opt.check_every : 10;
  BAE_HIP(hipMemcpyAsync(w.state.p, &h0, sizeof(h0), hipMemcpyHostToDevice, s));
  BAE_HIP(hipMemsetAsync(w.status.p, 0, 2 * sizeof(int32_t), s));
  BAE_HIP(hipMemsetAsync(w.x.p, 0, (size_t)ld * sizeof(double), s));
  BAE_HIP(hipMemsetAsync(w.p.p, 0, (size_t)ld * sizeof(double), s));
  BAE_HIP(hipMemsetAsync(w.minv.p, 0, (size_t)ld * 16 * sizeof(double), s));
  BAE_HIP(ev.record(1, s));
  if (nblocks)
    hipLaunchKernelGGL(k_pcg_blocks, dim3((nblocks + 3) / 4), dim3(64), 0, s, dA, ld, (const uint8_t*)w.nz.p, nt,
                       (const uint2*)w.blocks.p, nblocks, w.minv.p, w.status.p);
  BAE_HIP(ev.record(2, s));
  if (coarse) {
    BAE_HIP(ev.record(6, s));
    if ((rc = pcg_coarse_setup_device(e, dA, ld, plan))) return rc;
    BAE_HIP(ev.record(7, s));
  }
  PcgState hs = h0;
  double spmv_ms = 0.0, apply_ms = 0.0;
  uint32_t spmv_samples = 0, apply_samples = 0;
  const uint32_t max_passes = pcg_max_passes(h0.max_it);
  uint32_t k = 0;
  while (k < max_passes) {
    const uint32_t batch_end = std::min(max_passes, k + check_every);
    bool sampled = false, sampled_c = false;
    for (; k < batch_end; ++k) {
      const PcgState* sin = w.state.p + (k & 1);
      PcgState* sout = w.state.p + ((k + 1) & 1);
      const double* rin = w.r.p + (size_t)(k & 1) * ld;
      double* rout = w.r.p + (size_t)((k + 1) & 1) * ld;
      if (k > 0) {
        const bool sample = !sampled;
        if (sample) BAE_HIP(ev.record(3, s));
        hipLaunchKernelGGL(k_pcg_spmv_tiles, dim3(plan.n_tiles), dim3(256), 0, s, dA, ld, (const uint2*)w.tiles.p,
                           (const double*)w.p.p, (const double*)w.x.p, sin, w.rowslot.p, w.colslot.p);
        hipLaunchKernelGGL(k_pcg_spmv_gather, dim3(nt), dim3(64), 0, s, (const uint32_t*)w.row_ptr.p, (const uint32_t*)w.col_ptr.p,
                           (const uint32_t*)w.col_slot.p, (const double*)w.rowslot.p, (const double*)w.colslot.p,
                           (const double*)w.p.p, sin, w.q.p, pq_part);
        if (sample) { BAE_HIP(ev.record(4, s)); sampled = true; }
      }
      hipLaunchKernelGGL(k_pcg_update1, dim3(nb), dim3(256), 0, s, n, ld, nt, sin, (const double*)pq_part, d_rhs,
                         (const double*)w.q.p, rin, (const uint2*)w.blk.p, (const double*)w.minv.p, rout, w.z.p, rz_part, rr_part);
      if (coarse) {
        const bool sample = !sampled_c;
        if (sample) BAE_HIP(ev.record(8, s));
        pcg_coarse_apply_device(e, plan, sin, rout);
        if (sample) { BAE_HIP(ev.record(9, s)); sampled_c = true; }
        hipLaunchKernelGGL(k_pcg_update2<true>, dim3(nb), dim3(256), 0, s, ld, nt, nb, sin, sout, (const int32_t*)w.status.p,
                           (const double*)pq_part, (const double*)rz_part, (const double*)rr_part, (const double*)w.z.p, w.x.p,
                           w.p.p, nc, (const uint32_t*)w.cmap.p, (const double*)w.yc.p, (const double*)w.ryc_part.p);
      } else {
        hipLaunchKernelGGL(k_pcg_update2<false>, dim3(nb), dim3(256), 0, s, ld, nt, nb, sin, sout, (const int32_t*)w.status.p,
                           (const double*)pq_part, (const double*)rz_part, (const double*)rr_part, (const double*)w.z.p, w.x.p,
                           w.p.p, 0u, (const uint32_t*)nullptr, (const double*)nullptr, (const double*)nullptr);
      }
    }
    BAE_HIP(hipGetLastError());
    BAE_HIP(hipMemcpyAsync(&hs, w.state.p + (k & 1), sizeof(hs), hipMemcpyDeviceToHost, s));
    BAE_HIP(hipStreamSynchronize(s));
    if (sampled) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[3], ev[4]) == hipSuccess) { spmv_ms += ms; spmv_samples++; }
    }
    if (sampled_c) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[8], ev[9]) == hipSuccess) { apply_ms += ms; apply_samples++; }
    }
    if (hs.done) break;
  }
  BAE_HIP(hipMemcpyAsync(dx, w.x.p, (size_t)ld * sizeof(double), hipMemcpyDeviceToDevice, s));
  BAE_HIP(ev.record(5, s));
  BAE_HIP(hipStreamSynchronize(s));
  e->held.pcg_run_finished(coarse);
  if (coarse) {
    ba_hip_pcg_coarse_stats& c = e->pcg_coarse_stats;
    memset(&c, 0, sizeof(c));
    c.aggregate_used = plan.coarse_g; c.coarse_unknowns = nc; c.aggregates = plan.naggr;
    c.setup_ms = ev.ms(6, 7);
    c.apply_ms = apply_samples ? apply_ms / apply_samples : 0.0;
    c.coarse_bytes = 8.0 * (4.0 * ncp * ncp + 3.0 * ncp) + 4.0 * (plan.cmap.size() + plan.crow_ptr.size() + plan.crow_rows.size());
    w.coarse_nc = nc;
    w.coarse_ncp = ncp;
  }
  stats->iterations = hs.iterations; stats->converged = hs.converged; stats->residual_replacements = hs.replacements;
  stats->breakdown = hs.breakdown;
  stats->rhs_norm = sqrt(hs.bb);
  stats->rel_residual_recurrence = hs.bb > 0.0 ? sqrt(hs.rr_recur / hs.bb) : 0.0;
  stats->rel_residual_true = hs.bb > 0.0 ? sqrt(hs.rr_true / hs.bb) : 0.0;
  stats->solve_ms = ev.ms(0, 5); stats->precond_ms = ev.ms(1, 2);
  stats->spmv_ms = spmv_samples ? spmv_ms / spmv_samples : 0.0;
  stats->tiles_read_per_spmv = plan.n_tiles;
  stats->bytes_read_per_spmv = plan.bytes_per_spmv;
  *status = hs.breakdown ? 1 : 0;
  return 0;
}

}  // namespace bae
