// Joint covariance of an arbitrary parameter set from the factor that ba_hip_solve_gn leaves behind
// (ba_hip_get_joint_marginals): Sigma_sel,sel = Y^T D Y with Y = L^-1 E, a forward substitution over the
// reach of the requested tiles and a Gram product.  No selected inverse, no backward pass.
//
//   k_joint_init      Y panels of the reach = the unit columns E
//   k_joint_fsolve    partial tile sum_{J in chunk} L_IJ Y_J, one workgroup per (row I, chunk of <= 4 sources,
//                     block of 64 columns); one launch per level
//   k_joint_epilogue  Y_I = L_II^-1 (E_I - sum of the row's partial tiles in chunk order), one workgroup per
//                     (row I, block of 64 columns); one launch per level
//   k_joint_gram      partial tile sum_{I in group} Y_I^T D_I Y_I, one workgroup per (group of <= 8 reach rows,
//                     lower 64 x 64 tile of the output)
//   k_joint_combine   the groups summed in order, the lower half mirrored into the upper one
//
// The plan (reach, levels, chunks, slots) and the host restatement are in jointcov.h, checked on the CPU by
// tests/test_joint_marginals_plan.py.  The factor is read, never written: L_IJ from A, L_II^-T (linvT) and the
// pivot signs D from invdiag.  FP64, no atomics: every partial tile has one writer and the sums run in the
// plan's order, so two calls give the same bits.
//
// The tile products run on v_mfma_f64_16x16x4_f64 with the staging of tile_mma.h: four waves, each owning a
// 32x32 quarter of the output tile; operands go through LDS 32 k-rows at a time, k-major, and the next chunk
// is fetched into registers while the matrix cores work on this one.
#include "engine.h"
#include "jointcov.h"
#include "tile_mma.h"

#include <algorithm>
#include <vector>

namespace bae {

using namespace tile64;

// col_key[c]: 64 position + row inside the tile of the unit entry of column c (kJointNone for padding columns)
__global__ void __launch_bounds__(256)
k_joint_init(double* __restrict__ Y, uint64_t count, uint32_t mp, const uint32_t* __restrict__ col_key) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  Y[t] = col_key[t % mp] == (uint32_t)(t / mp) ? 1.0 : 0.0;
}

// chunks: (I, position of I, first source, end source) of one level; slot (blockIdx.x, blockIdx.y) = the
// partial tile sum_{J in chunk} L_IJ Y_J[:, 64 b .. 64 b + 64)
__global__ void __launch_bounds__(256)
k_joint_fsolve(const uint4* __restrict__ chunks, const uint32_t* __restrict__ src, const uint32_t* __restrict__ pos,
               const double* __restrict__ A, uint32_t ld, const double* __restrict__ Y, uint32_t mp,
               double* __restrict__ slots) {
  __shared__ Lds s;
  const uint4 c = chunks[blockIdx.x];
  const uint32_t I = c.x, s0 = c.z, b = blockIdx.y;
  const uint32_t nch = 2 * (c.w - s0);
  double4_t acc[2][2];
  zero_acc(acc);
  Chunk ca, cb;
  auto fetch = [&](uint32_t ch) {
    const uint32_t J = src[s0 + (ch >> 1)];
    const int k0 = KCH * (int)(ch & 1);
    load_imajor(ca, A + (size_t)I * TB * ld + (size_t)J * TB, ld, k0);              // X[k][r] = L_IJ[r][k]
    load_kmajor(cb, Y + (size_t)pos[J] * TB * mp + (size_t)b * TB, mp, k0);         // Y[k][x] = Y_J[k][x]
  };
  if (nch) fetch(0);
  for (uint32_t ch = 0; ch < nch; ++ch) {
    store_imajor(ca, s.X);
    store_kmajor(cb, s.Y);
    __syncthreads();
    if (ch + 1 < nch) fetch(ch + 1);
    mma_chunk(acc, s);
    __syncthreads();
  }
  store_tile(slots + ((size_t)blockIdx.x * gridDim.y + b) * (TB * TB), TB, acc);
}

// rows: (I, first chunk, end chunk, first chunk of the level) of one level.
// Y_I = L_II^-1 T, T = Y_I (the unit entries) - the row's partial tiles in chunk order.
__global__ void __launch_bounds__(256)
k_joint_epilogue(const uint4* __restrict__ rows, const uint32_t* __restrict__ pos, const double* __restrict__ linvT,
                 double* __restrict__ Y, uint32_t mp, const double* __restrict__ slots) {
  __shared__ Lds s;
  const uint4 r = rows[blockIdx.x];
  const uint32_t I = r.x, b = blockIdx.y, ncb = gridDim.y;
  double* YI = Y + (size_t)pos[I] * TB * mp + (size_t)b * TB;
  const double* G = linvT + (size_t)I * TB * TB;  // G[c][x] = (L_II^-1)[x][c]: X[k = c][i = x]
  const int tid = threadIdx.x;
  // T first, both 32-row halves at once.  Thread t owns elements e = t + 256 q of the 64 x 64 tile: the 16 loads
  // of a slot are independent and in flight together; each element subtracts its slots in chunk order
  double v[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) v[q] = YI[(size_t)((tid + 256 * q) / TB) * mp + tid % TB];
  const double* sl = slots + ((size_t)(r.y - r.w) * ncb + b) * (TB * TB) + tid;
  for (uint32_t c = r.y; c < r.z; ++c, sl += (size_t)ncb * (TB * TB)) {
    double w[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) w[q] = sl[256 * q];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] -= w[q];
  }
  double4_t out[2][2];
  zero_acc(out);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    Chunk cg;
    load_kmajor(cg, G, TB, KCH * h);
    store_kmajor(cg, s.X);
#pragma unroll
    for (int q = 0; q < 8; ++q) s.Y[(tid + 256 * q) / TB][tid % TB] = v[8 * h + q];
    __syncthreads();
    mma_chunk(out, s);
    __syncthreads();
  }
  store_tile(YI, mp, out);
}

// part[(g, t)] = sum_{q in group g} Y_q[:, bi]^T D_q Y_q[:, bj], t = bi (bi + 1) / 2 + bj, bi >= bj
__global__ void __launch_bounds__(256)
k_joint_gram(const double* __restrict__ Y, uint32_t mp, const uint32_t* __restrict__ reach, uint32_t nr,
             const double* __restrict__ dsgn, double* __restrict__ part) {
  __shared__ Lds s;
  const uint32_t g = blockIdx.x, t = blockIdx.y;
  uint32_t bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
  const uint32_t bj = t - bi * (bi + 1) / 2;
  const uint32_t q0 = g * kJointGramGroup, q1 = min(nr, q0 + kJointGramGroup);
  const uint32_t nch = 2 * (q1 - q0);
  const int tid = threadIdx.x;
  double4_t acc[2][2];
  zero_acc(acc);
  Chunk ca, cb;
  auto fetch = [&](uint32_t ch) {
    const uint32_t q = q0 + (ch >> 1);
    const int k0 = KCH * (int)(ch & 1);
    const double* Yq = Y + (size_t)q * TB * mp;
    load_kmajor(ca, Yq + (size_t)bi * TB, mp, k0);
    load_kmajor(cb, Yq + (size_t)bj * TB, mp, k0);
    const double* d = dsgn + (size_t)reach[q] * TB + k0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const double dk = d[(2 * tid + 512 * x) / TB];
      ca.v[x].x *= dk;
      ca.v[x].y *= dk;
    }
  };
  if (nch) fetch(0);
  for (uint32_t ch = 0; ch < nch; ++ch) {
    store_kmajor(ca, s.X);
    store_kmajor(cb, s.Y);
    __syncthreads();
    if (ch + 1 < nch) fetch(ch + 1);
    mma_chunk(acc, s);
    __syncthreads();
  }
  store_tile(part + ((size_t)g * gridDim.y + t) * (TB * TB), TB, acc);
}

// out (M x M): the groups in order; the lower half is computed and mirrored
__global__ void __launch_bounds__(256)
k_joint_combine(const double* __restrict__ part, uint32_t groups, uint32_t ntl, uint32_t M, double* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)M * M) return;
  const uint32_t a = (uint32_t)(t / M), b = (uint32_t)(t % M);
  if (b > a) return;
  const uint32_t bi = a / TB, bj = b / TB, tl = bi * (bi + 1) / 2 + bj;
  const size_t off = (size_t)(a % TB) * TB + b % TB;
  double sum = 0.0;
  for (uint32_t g = 0; g < groups; ++g) sum += part[((size_t)g * ntl + tl) * (TB * TB) + off];
  out[(size_t)a * M + b] = sum;
  out[(size_t)b * M + a] = sum;
}

// ---- host side ----------------------------------------------------------------------------------------
// sel: the requested rows of S in the engine's (factorised) numbering, out: M x M on the host
int jointcov_run(Engine* e, const std::vector<uint32_t>& sel, double* out) {
  const Structure& st = e->st;
  const uint32_t M = (uint32_t)sel.size();
  uint32_t nt;
  const double *dsgn, *linvT;
  if (int rc = kept_factor(e, "joint marginals", &nt, &dsgn, &linvT)) return rc;
  std::vector<uint32_t> tiles(M);
  for (uint32_t c = 0; c < M; ++c) tiles[c] = sel[c] / TB;
  JointPlan p;
  build_joint_plan(e->nzL_host, nt, tiles, M, p);
  const uint32_t nr = (uint32_t)p.reach.size(), mp = p.m_pad, ncb = p.ncb, ntl = ncb * (ncb + 1) / 2;
  // one index buffer: chunks | rows (both read as uint4) | src | pos | reach | col_key
  std::vector<uint32_t> idx;
  const size_t o_chunks = 0, o_rows = p.chunks.size(), o_src = o_rows + p.rows.size(), o_pos = o_src + p.src.size(),
               o_reach = o_pos + nt, o_key = o_reach + nr;
  idx.reserve(o_key + mp);
  idx.insert(idx.end(), p.chunks.begin(), p.chunks.end());
  idx.insert(idx.end(), p.rows.begin(), p.rows.end());
  idx.insert(idx.end(), p.src.begin(), p.src.end());
  idx.insert(idx.end(), p.pos.begin(), p.pos.end());
  idx.insert(idx.end(), p.reach.begin(), p.reach.end());
  for (uint32_t c = 0; c < mp; ++c) idx.push_back(c < M ? p.pos[sel[c] / TB] * TB + sel[c] % TB : kJointNone);
  const size_t n_y = p.y_count(), n_slots = (size_t)std::max(p.max_level_chunks, 1u) * ncb * TB * TB,
               n_part = (size_t)p.gram_groups * ntl * TB * TB, n_out = (size_t)M * M;
  const size_t bytes = (n_y + n_slots + n_part + n_out) * sizeof(double) + idx.size() * sizeof(uint32_t);
  if (e->jc_idx.alloc(idx.size()) != hipSuccess || e->jc_Y.alloc(n_y) != hipSuccess ||
      e->jc_slots.alloc(n_slots) != hipSuccess || e->jc_part.alloc(n_part) != hipSuccess ||
      e->jc_out.alloc(n_out) != hipSuccess) {
    (void)hipGetLastError();
    jointcov_release(e);
    char msg[160];
    snprintf(msg, sizeof msg, "joint marginals: allocating the workspace (%zu bytes, %u reach tiles, %u columns) failed",
             bytes, nr, M);
    return e->fail_msg(msg);
  }
  BAE_HIP(hipMemcpy(e->jc_idx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  const uint32_t* d_idx = e->jc_idx.p;
  const uint4* d_chunks = reinterpret_cast<const uint4*>(d_idx + o_chunks);
  const uint4* d_rows = reinterpret_cast<const uint4*>(d_idx + o_rows);
  Events<3> ev;
  BAE_HIP(ev.create());
  (void)ev.record(0, e->stream);
  hipLaunchKernelGGL(k_joint_init, dim3((unsigned)((n_y + 255) / 256)), dim3(256), 0, e->stream, e->jc_Y.p, (uint64_t)n_y,
                     mp, d_idx + o_key);
  for (uint32_t v = 0; v < p.levels(); ++v) {
    const uint32_t c0 = p.chunk_level_ptr[v], c1 = p.chunk_level_ptr[v + 1];
    if (c1 > c0)
      hipLaunchKernelGGL(k_joint_fsolve, dim3(c1 - c0, ncb), dim3(256), 0, e->stream, d_chunks + c0, d_idx + o_src,
                         d_idx + o_pos, (const double*)e->A.p, st.ld, (const double*)e->jc_Y.p, mp, e->jc_slots.p);
    const uint32_t r0 = p.level_ptr[v], r1 = p.level_ptr[v + 1];
    hipLaunchKernelGGL(k_joint_epilogue, dim3(r1 - r0, ncb), dim3(256), 0, e->stream, d_rows + r0, d_idx + o_pos, linvT,
                       e->jc_Y.p, mp, (const double*)e->jc_slots.p);
  }
  (void)ev.record(1, e->stream);
  hipLaunchKernelGGL(k_joint_gram, dim3(p.gram_groups, ntl), dim3(256), 0, e->stream, (const double*)e->jc_Y.p, mp,
                     d_idx + o_reach, nr, dsgn, e->jc_part.p);
  hipLaunchKernelGGL(k_joint_combine, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, e->stream,
                     (const double*)e->jc_part.p, p.gram_groups, ntl, M, e->jc_out.p);
  (void)ev.record(2, e->stream);
  const hipError_t lerr = hipGetLastError();
  const hipError_t serr = hipEventSynchronize(ev[2]);
  ba_hip_joint_marginal_stats js = {};
  js.solve_ms = ev.ms(0, 1);
  js.gram_ms = ev.ms(1, 2);
  if (lerr != hipSuccess) return e->fail(lerr, "k_joint launch");
  if (serr != hipSuccess) return e->fail(serr, "k_joint");
  BAE_HIP(hipMemcpy(out, e->jc_out.p, n_out * sizeof(double), hipMemcpyDeviceToHost));
  js.columns = M;
  js.reach_tiles = nr;
  js.levels = p.levels();
  js.tile_products = p.products;
  js.workspace_bytes = (double)(e->jc_idx.bytes() + e->jc_Y.bytes() + e->jc_slots.bytes() + e->jc_part.bytes() +
                                e->jc_out.bytes());
  e->jstats = js;
  return 0;
}

void jointcov_release(Engine* e) {   // (ba_hip_release_marginals promises the memory back while the engine lives)
  e->jc_idx.release(); e->jc_Y.release(); e->jc_slots.release(); e->jc_part.release(); e->jc_out.release();
}

}  // namespace bae
