// Panel PCG: m <= 512 independent block-Jacobi PCG recurrences on S in lock-step (pcg_panel.h has the algorithm,
// the plan and the host restatement).  Panels are (64 nt) x m_pad row-major.  One pass is six launches:
//
//   k_pcgp_spmm           partial tile sum over a chunk of <= 8 sources of tile row I, one workgroup per (chunk, block
//                         of 64 columns): A_IJ P_J (A_IJ index-major), the symmetrised diagonal tile, A_I'I^T P_I'
//                         (A_I'I k-major); the next 32 k-rows are fetched under the MFMAs of these
//   k_pcgp_spmm_epilogue  Q_I = the slots of tile row I in chunk order, and the per-column partials of p.q
//   k_pcgp_alpha          one thread per column: p.q over the tile rows in ascending order, alpha_j for update1
//   k_pcgp_update1        r <- r - alpha_j q (r <- b, r <- b - q), z = M^-1 r, per-column partials of r.z and r.r
//   k_pcgp_decide         one thread per column: the sums, pcg_decide, the next state into the other copy, the
//                         all-done word and one word per column block
//   k_pcgp_update2        x += alpha_j p, p = z + beta_j p (p = z, p = x), every column masked by its action bits
//
// and k_panel_scatter / k_panel_gather (k_factorsolve.hip) move the caller's B and X between the host layout and the
// panels.  Every kernel of a pass but k_pcgp_decide returns at once when the all-done word (or the word of its column
// block) is set, so the host enqueues check_every passes blind and reads one word back per batch.  FP64; the tile
// products run on v_mfma_f64_16x16x4_f64 with the staging of tile_mma.h; no atomics, no memory-side adds, every sum
// in a fixed order.
#include "engine.h"
#include "pcg_panel.h"
#include "tile_mma.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace bae {

using namespace tile64;

// k_pcg.hip: the inverses of the preconditioner's blocks
__global__ void k_pcg_blocks(const double* __restrict__ A, uint32_t ld, const uint8_t* __restrict__ nz, uint32_t nt,
                             const uint2* __restrict__ blocks, uint32_t nblocks, double* __restrict__ minv,
                             int32_t* __restrict__ status);

// flags: [0] every column is done, [1 + b] every column of block b is done
static __device__ __forceinline__ bool pcgp_idle(const uint32_t* __restrict__ flags, uint32_t b) {
  return flags[0] != 0 || flags[1 + b] != 0;
}

// 32 k-columns of the symmetric diagonal tile in the index-major layout of load_imajor, from its lower triangle:
// element (i, k) is read at (max, min)
static __device__ __forceinline__ void load_diag_sym(Chunk& c, const double* __restrict__ src, size_t ld, int k0) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int e = 2 * tid + 512 * s;
    const int i = e / KCH, k = k0 + e % KCH;
    c.v[s].x = src[(size_t)max(i, k) * ld + min(i, k)];
    c.v[s].y = src[(size_t)max(i, k + 1) * ld + min(i, k + 1)];
  }
}

// chunks: (I, first source, end source, -); src: (tile index, kind).  Slot (blockIdx.x, b) = the partial tile of the
// chunk for the column block b.
__global__ void __launch_bounds__(256)
k_pcgp_spmm(const uint4* __restrict__ chunks, const uint2* __restrict__ src, const double* __restrict__ A, uint32_t ld,
            const double* __restrict__ P, uint32_t mp, const uint32_t* __restrict__ flags, double* __restrict__ slots) {
  const uint32_t b = blockIdx.y;
  if (pcgp_idle(flags, b)) return;
  __shared__ Lds s;
  const uint4 c = chunks[blockIdx.x];
  const uint32_t I = c.x, s0 = c.y;
  const uint32_t nch = 2 * (c.z - s0);
  double4_t acc[2][2];
  zero_acc(acc);
  Chunk ca, cb;
  auto fetch = [&](uint32_t ch) {
    const uint2 sr = src[s0 + (ch >> 1)];
    const int k0 = KCH * (int)(ch & 1);
    if (sr.y == kPanelCol) load_kmajor(ca, A + (size_t)sr.x * TB * ld + (size_t)I * TB, ld, k0);        // X[k][i] = A_I'I[k][i]
    else if (sr.y == kPanelRow) load_imajor(ca, A + (size_t)I * TB * ld + (size_t)sr.x * TB, ld, k0);   // X[k][i] = A_IJ[i][k]
    else load_diag_sym(ca, A + (size_t)I * TB * ld + (size_t)I * TB, ld, k0);
    load_kmajor(cb, P + (size_t)sr.x * TB * mp + (size_t)b * TB, mp, k0);                               // Y[k][j] = P_T[k][j]
  };
  // (not accumulate_chunks: through it the same instructions come out in another order, and a product that takes
  // 84 us at 1000 poses and up to 64 columns takes 87 to 90; profiles/tile_pipeline_ab.txt has the three-library run)
  if (nch) fetch(0);
  for (uint32_t ch = 0; ch < nch; ++ch) {
    if (src[s0 + (ch >> 1)].y == kPanelCol) store_kmajor(ca, s.X);
    else store_imajor(ca, s.X);
    store_kmajor(cb, s.Y);
    __syncthreads();
    if (ch + 1 < nch) fetch(ch + 1);
    mma_chunk(acc, s);
    __syncthreads();
  }
  store_tile(slots + ((size_t)blockIdx.x * gridDim.y + b) * (TB * TB), TB, acc);
}

// Thread t owns the elements e = t + 256 q of a 64 x 64 tile: column t & 63, rows (t >> 6) + 4 q.  The sum of a
// column over the 64 rows: the thread's 16 rows in ascending order, then (s0 + s2) + (s1 + s3) (pcg_panel_colsum).
static __device__ __forceinline__ double pcgp_colsum(double s, double (*red)[64]) {
  const uint32_t col = threadIdx.x & 63u, rs = threadIdx.x >> 6;
  red[rs][col] = s;
  __syncthreads();
  const double v = (red[0][col] + red[2][col]) + (red[1][col] + red[3][col]);
  __syncthreads();
  return v;
}

__global__ void __launch_bounds__(256)
k_pcgp_spmm_epilogue(const uint32_t* __restrict__ chunk_ptr, const double* __restrict__ slots, const double* __restrict__ P,
                     uint32_t mp, const uint32_t* __restrict__ flags, double* __restrict__ Q, double* __restrict__ pq_part) {
  const uint32_t I = blockIdx.x, b = blockIdx.y, ncb = gridDim.y;
  if (pcgp_idle(flags, b)) return;
  __shared__ double red[4][64];
  const uint32_t tid = threadIdx.x, col = tid & 63u, rs = tid >> 6;
  double v[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) v[q] = 0.0;
  const uint32_t c0 = chunk_ptr[I], c1 = chunk_ptr[I + 1];
  const double* sl = slots + ((size_t)c0 * ncb + b) * (TB * TB) + tid;
  for (uint32_t c = c0; c < c1; ++c, sl += (size_t)ncb * (TB * TB)) {
    double w[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) w[q] = sl[256 * q];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] += w[q];
  }
  double sum = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const size_t off = ((size_t)I * TB + rs + 4 * q) * mp + (size_t)b * TB + col;
    Q[off] = v[q];
    sum += P[off] * v[q];
  }
  const double t = pcgp_colsum(sum, red);
  if (tid < 64) pq_part[(size_t)I * mp + (size_t)b * TB + tid] = t;
}

// The partials of one column over the tile rows, added in ascending order.  One thread owns the whole sum (the
// order is the restatement's), so the loads are what it waits for: sixteen are in flight before the first add.
static __device__ __forceinline__ double pcgp_rows_sum(const double* __restrict__ part, uint32_t nt, uint32_t mp) {
  double sum = 0.0;
  uint32_t I = 0;
  for (; I + 16 <= nt; I += 16) {
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = part[(size_t)(I + u) * mp];
#pragma unroll
    for (int u = 0; u < 16; ++u) sum += v[u];
  }
  for (; I < nt; ++I) sum += part[(size_t)I * mp];
  return sum;
}

// colv: pq | alpha1 (update1) | alpha2 | beta (update2), m_pad each; colu: act | run, m_pad each
__global__ void __launch_bounds__(256)
k_pcgp_alpha(uint32_t nt, uint32_t mp, const PcgState* __restrict__ st, const double* __restrict__ pq_part,
             const uint32_t* __restrict__ flags, double* __restrict__ pq, double* __restrict__ alpha1,
             uint32_t* __restrict__ run) {
  if (flags[0]) return;
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= mp) return;
  const PcgState s = st[j];
  double sum = 0.0, a = 0.0;
  bool go = !s.done;
  if (!s.done && s.mode == kPcgIter) {
    sum = pcgp_rows_sum(pq_part + j, nt, mp);
    a = s.rz_old / sum;
    go = pcg_finite(sum) && sum > 0.0 && pcg_finite(a);   // otherwise update1 leaves the column alone: decide reports it
  }
  pq[j] = sum;
  alpha1[j] = a;
  run[j] = go ? 1u : 0u;
}

// One workgroup per (tile row, column block).  r is double buffered as in k_pcg_update1: z = M^-1 r reads the rows
// of the whole preconditioner block, which other workgroups write.
__global__ void __launch_bounds__(256)
k_pcgp_update1(uint32_t n, uint32_t mp, const PcgState* __restrict__ st, const double* __restrict__ alpha1,
               const uint32_t* __restrict__ run, const double* __restrict__ B, const double* __restrict__ Q,
               const double* __restrict__ r_in, const uint2* __restrict__ blk, const double* __restrict__ minv,
               const uint32_t* __restrict__ flags, double* __restrict__ r_out, double* __restrict__ Z,
               double* __restrict__ rz_part, double* __restrict__ rr_part) {
  const uint32_t I = blockIdx.x, b = blockIdx.y;
  if (pcgp_idle(flags, b)) return;
  __shared__ double red[4][64];
  const uint32_t tid = threadIdx.x, col = tid & 63u, rs = tid >> 6;
  const uint32_t j = b * TB + col;
  const uint32_t mode = st[j].mode;
  const bool go = run[j] != 0;
  const double a = alpha1[j];
  double sz = 0.0, sr = 0.0;
  if (go) {
    for (int q = 0; q < 16; ++q) {
      const size_t row = (size_t)I * TB + rs + 4 * q;
      double rn = 0.0, zz = 0.0;
      if (row < n) {
        const uint2 bl = blk[row];
        for (uint32_t t = 0; t < bl.y; ++t) {
          const size_t c = bl.x + t, off = c * mp + j;
          const double rj = mode == kPcgIter ? r_in[off] - a * Q[off] : mode == kPcgInit ? B[off] : B[off] - Q[off];
          if (c == row) rn = rj;
          zz += minv[row * 16 + t] * rj;
        }
      }
      r_out[row * mp + j] = rn;
      Z[row * mp + j] = zz;
      sz += rn * zz;
      sr += rn * rn;
    }
  }
  const double tz = pcgp_colsum(sz, red);
  const double tr = pcgp_colsum(sr, red);
  if (tid < 64 && go) {
    rz_part[(size_t)I * mp + j] = tz;
    rr_part[(size_t)I * mp + j] = tr;
  }
}

// One workgroup.  It runs in every pass, also when all columns are done: both copies of the state then hold the end.
__global__ void __launch_bounds__(256)
k_pcgp_decide(uint32_t nt, uint32_t mp, const PcgState* __restrict__ st, PcgState* __restrict__ st_out,
              const int32_t* __restrict__ status, const double* __restrict__ pq, const double* __restrict__ rz_part,
              const double* __restrict__ rr_part, const uint32_t* __restrict__ run, uint32_t* __restrict__ flags_out,
              double* __restrict__ alpha2, double* __restrict__ beta, uint32_t* __restrict__ act) {
  __shared__ uint32_t open[kPcgPanelMaxColumns / 64 + 1];
  const uint32_t tid = threadIdx.x, ncb = mp / TB;
  if (tid <= ncb) open[tid] = 0;
  __syncthreads();
  const int block_status = status[0];
  for (uint32_t j = tid; j < mp; j += 256) {
    const PcgState s = st[j];
    PcgState o = s;
    double a = 0.0, be = 0.0;
    uint32_t ac = 0;
    if (!s.done) {
      double rz = 0.0, rr = 0.0;
      if (run[j]) {
        rz = pcgp_rows_sum(rz_part + j, nt, mp);
        rr = pcgp_rows_sum(rr_part + j, nt, mp);
      }
      ac = pcg_decide(s, pq[j], rz, rr, block_status, o, a, be);
      if (!o.done && o.mode == kPcgVerify) ac |= kPcgPanelToX;
    }
    st_out[j] = o;
    alpha2[j] = a;
    beta[j] = be;
    act[j] = ac;
    if (!o.done) { open[0] = 1; open[1 + j / TB] = 1; }   // every writer stores the same value
  }
  __syncthreads();
  if (tid <= ncb) flags_out[tid] = open[tid] ? 0u : 1u;
}

__global__ void __launch_bounds__(256)
k_pcgp_update2(uint32_t mp, const uint32_t* __restrict__ act, const double* __restrict__ alpha2, const double* __restrict__ beta,
               const double* __restrict__ Z, const uint32_t* __restrict__ flags, double* __restrict__ X, double* __restrict__ P) {
  const uint32_t I = blockIdx.x, b = blockIdx.y;
  if (pcgp_idle(flags, b)) return;
  const uint32_t tid = threadIdx.x, col = tid & 63u, rs = tid >> 6;
  const uint32_t j = b * TB + col;
  const uint32_t ac = act[j];
  if (!ac) return;   // frozen, or a pass that moves nothing
  const double a = alpha2[j], be = beta[j];
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const size_t off = ((size_t)I * TB + rs + 4 * q) * mp + j;
    const double pv = P[off];
    double xv = X[off];
    if (ac & kPcgStep) { xv += a * pv; X[off] = xv; }
    if (ac & kPcgDir) P[off] = Z[off] + be * pv;
    else if (ac & kPcgRestart) P[off] = Z[off];
    if (ac & kPcgPanelToX) P[off] = xv;
  }
}

int pcg_panel_solve_device(Engine* e, const double* dA, uint32_t n, uint32_t ld, const PcgPlan& plan,
                           const std::vector<uint8_t>& nz, const std::vector<uint32_t>& blk, const std::vector<uint32_t>& blocks,
                           const uint32_t* rowmap, uint32_t m, const double* B, double* X, const ba_hip_pcg_options& opt,
                           int* status) {
  Engine::PcgPanelWork& w = e->pcgp;
  hipStream_t s = e->stream;
  const uint32_t nt = plan.nt, nblocks = (uint32_t)(blocks.size() / 2);
  *status = 0;
  if (ld != 64 * nt || blk.size() != (size_t)2 * ld || nz.size() != (size_t)nt * nt || m == 0 || m > kPcgPanelMaxColumns || n > ld)
    return e->fail_msg("pcg_panel_solve_device: plan does not match the system");
  PcgPanelPlan pp;
  build_pcg_panel_plan(plan, m, pp);
  const uint32_t mp = pp.m_pad, ncb = pp.ncb, nflag = 1 + ncb;
  const size_t N = (size_t)ld * mp, n_io = (size_t)n * m;
  IndexPack idx;   // the tables in one buffer
  const size_t o_ch = idx.add(pp.chunks, 4), o_src = idx.add(pp.src, 2), o_blk = idx.add(blk, 2), o_blocks = idx.add(blocks, 2),
               o_cp = idx.add(pp.chunk_ptr, 4), o_map = idx.add(rowmap, rowmap + ld);
  Events<4> ev;   // 0 / 3 the solve, 1 / 2 one product of a batch
  BAE_HIP(ev.create());
  int rc;
  if ((rc = idx.upload_async(e, w.idx)) || (rc = upload_async(e, w.nz, nz.data(), nz.size()))) return rc;
  BAE_HIP(w.stage.alloc(n_io));
  BAE_HIP(w.B.alloc(N)); BAE_HIP(w.X.alloc(N)); BAE_HIP(w.P.alloc(N)); BAE_HIP(w.Z.alloc(N)); BAE_HIP(w.Q.alloc(N));
  BAE_HIP(w.R.alloc(2 * N));
  BAE_HIP(w.slots.alloc(std::max(pp.slot_doubles(), (size_t)1)));
  BAE_HIP(w.minv.alloc((size_t)ld * 16));
  BAE_HIP(w.parts.alloc((size_t)3 * nt * mp));
  BAE_HIP(w.colv.alloc((size_t)4 * mp));
  BAE_HIP(w.colu.alloc((size_t)2 * mp + 2 * nflag));
  BAE_HIP(w.state.alloc((size_t)2 * mp));
  BAE_HIP(w.status.alloc(2));
  const uint4* d_chunks = idx.at<uint4>(o_ch);
  const uint2 *d_src = idx.at<uint2>(o_src), *d_blk = idx.at<uint2>(o_blk), *d_blocks = idx.at<uint2>(o_blocks);
  const uint32_t *d_cp = idx.at(o_cp), *d_map = idx.at(o_map);
  double *pq_part = w.parts.p, *rz_part = pq_part + (size_t)nt * mp, *rr_part = rz_part + (size_t)nt * mp;
  double *pq = w.colv.p, *alpha1 = pq + mp, *alpha2 = alpha1 + mp, *beta = alpha2 + mp;
  uint32_t *act = w.colu.p, *run = act + mp, *flags = run + mp;   // flags: two copies of nflag words
  PcgState h0;
  memset(&h0, 0, sizeof(h0));
  h0.tol2 = opt.rel_tolerance * opt.rel_tolerance;
  h0.max_it = opt.max_iterations ? opt.max_iterations : n;
  h0.mode = kPcgInit;
  const std::vector<PcgState> init(mp, h0);
  const uint32_t check_every = opt.check_every ? opt.check_every : 10;
  BAE_HIP(hipMemcpyAsync(w.stage.p, B, n_io * sizeof(double), hipMemcpyHostToDevice, s));
  BAE_HIP(hipMemcpyAsync(w.state.p, init.data(), (size_t)mp * sizeof(PcgState), hipMemcpyHostToDevice, s));
  BAE_HIP(ev.record(0, s));
  BAE_HIP(hipMemsetAsync(w.status.p, 0, 2 * sizeof(int32_t), s));
  BAE_HIP(hipMemsetAsync(w.colu.p, 0, ((size_t)2 * mp + 2 * nflag) * sizeof(uint32_t), s));
  BAE_HIP(hipMemsetAsync(w.X.p, 0, N * sizeof(double), s));
  BAE_HIP(hipMemsetAsync(w.P.p, 0, N * sizeof(double), s));
  BAE_HIP(hipMemsetAsync(w.minv.p, 0, (size_t)ld * 16 * sizeof(double), s));
  panel_scatter_launch(s, w.stage.p, m, d_map, (uint64_t)N, mp, w.B.p);
  if (nblocks)
    hipLaunchKernelGGL(k_pcg_blocks, dim3((nblocks + 3) / 4), dim3(64), 0, s, dA, ld, (const uint8_t*)w.nz.p, nt, d_blocks,
                       nblocks, w.minv.p, w.status.p);
  const dim3 g_tiles(nt, ncb), g_spmm(pp.n_chunks(), ncb);
  uint32_t done = 0;
  double spmm_ms = 0.0;
  uint32_t spmm_samples = 0;
  const uint32_t max_passes = pcg_max_passes(h0.max_it);
  uint32_t k = 0;
  while (k < max_passes) {
    const uint32_t batch_end = std::min(max_passes, k + check_every);
    bool sampled = false;
    for (; k < batch_end; ++k) {
      const PcgState* sin = w.state.p + (size_t)(k & 1) * mp;
      PcgState* sout = w.state.p + (size_t)((k + 1) & 1) * mp;
      const uint32_t* fin = flags + (size_t)(k & 1) * nflag;
      uint32_t* fout = flags + (size_t)((k + 1) & 1) * nflag;
      const double* rin = w.R.p + (size_t)(k & 1) * N;
      double* rout = w.R.p + (size_t)((k + 1) & 1) * N;
      if (k > 0) {
        const bool sample = !sampled;
        if (sample) BAE_HIP(ev.record(1, s));
        hipLaunchKernelGGL(k_pcgp_spmm, g_spmm, dim3(256), 0, s, d_chunks, d_src, dA, ld, (const double*)w.P.p, mp, fin, w.slots.p);
        hipLaunchKernelGGL(k_pcgp_spmm_epilogue, g_tiles, dim3(256), 0, s, d_cp, (const double*)w.slots.p, (const double*)w.P.p,
                           mp, fin, w.Q.p, pq_part);
        if (sample) { BAE_HIP(ev.record(2, s)); sampled = true; }
      }
      hipLaunchKernelGGL(k_pcgp_alpha, dim3((mp + 255) / 256), dim3(256), 0, s, nt, mp, sin, (const double*)pq_part, fin, pq,
                         alpha1, run);
      hipLaunchKernelGGL(k_pcgp_update1, g_tiles, dim3(256), 0, s, n, mp, sin, (const double*)alpha1, (const uint32_t*)run,
                         (const double*)w.B.p, (const double*)w.Q.p, rin, d_blk, (const double*)w.minv.p, fin, rout, w.Z.p,
                         rz_part, rr_part);
      hipLaunchKernelGGL(k_pcgp_decide, dim3(1), dim3(256), 0, s, nt, mp, sin, sout, (const int32_t*)w.status.p,
                         (const double*)pq, (const double*)rz_part, (const double*)rr_part, (const uint32_t*)run, fout, alpha2,
                         beta, act);
      hipLaunchKernelGGL(k_pcgp_update2, g_tiles, dim3(256), 0, s, mp, (const uint32_t*)act, (const double*)alpha2,
                         (const double*)beta, (const double*)w.Z.p, fin, w.X.p, w.P.p);
    }
    BAE_HIP(hipGetLastError());
    BAE_HIP(hipMemcpyAsync(&done, flags + (size_t)(k & 1) * nflag, sizeof(done), hipMemcpyDeviceToHost, s));
    BAE_HIP(hipStreamSynchronize(s));
    if (sampled) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) { spmm_ms += ms; spmm_samples++; }
    }
    if (done) break;
  }
  panel_gather_launch(s, w.X.p, mp, d_map, (uint64_t)N, m, w.stage.p);
  BAE_HIP(ev.record(3, s));
  BAE_HIP(hipGetLastError());
  std::vector<PcgState> cols(mp);
  BAE_HIP(hipMemcpyAsync(cols.data(), w.state.p + (size_t)(k & 1) * mp, (size_t)mp * sizeof(PcgState), hipMemcpyDeviceToHost, s));
  BAE_HIP(hipMemcpyAsync(X, w.stage.p, n_io * sizeof(double), hipMemcpyDeviceToHost, s));
  BAE_HIP(hipStreamSynchronize(s));
  cols.resize(m);
  ba_hip_pcg_panel_stats st;
  memset(&st, 0, sizeof(st));
  st.columns = m; st.column_blocks = ncb; st.passes = k;
  for (const PcgState& c : cols) {
    if (c.breakdown) st.broken_down++;
    else if (c.converged) st.converged++;
    else st.capped++;
    if (!c.breakdown && c.bb > 0.0) st.max_rel_residual_true = std::max(st.max_rel_residual_true, sqrt(c.rr_true / c.bb));
  }
  st.solve_ms = ev.ms(0, 3);
  st.spmm_ms = spmm_samples ? spmm_ms / spmm_samples : 0.0;
  st.tile_products_per_pass = pp.products();
  st.bytes_read_per_product = pp.bytes_read();
  st.workspace_bytes = (double)w.bytes();
  e->pcgp_stats = st;
  e->pcgp_cols = cols;
  *status = st.broken_down ? 1 : 0;
  return 0;
}

}  // namespace bae
