// Joint covariance of an arbitrary parameter set from the factor that ba_hip_solve_gn leaves behind
// (ba_hip_get_joint_marginals): Sigma_sel,sel = Y^T D Y with Y = L^-1 E, a forward substitution over the
// reach of the requested tiles and a Gram product.  No selected inverse, no backward pass.
//
//   k_joint_init      Y panels of the reach = the unit columns E
//   k_joint_seed      (landmark columns, ba_hip_get_joint_state_marginals) the tile rows the valid incidences of
//                     every requested landmark touch, one wavefront per landmark; the host seeds the plan with them
//   k_joint_rhs       the landmark columns -W_l V_l^-1 added into the Y panels, one wavefront per landmark, a fixed
//                     lane per entry, incidences in lm_entry's order
//   k_joint_fsolve    partial tile sum_{J in chunk} L_IJ Y_J, one workgroup per (row I, chunk of <= 4 sources,
//                     block of 64 columns); one launch per level
//   k_joint_epilogue  Y_I = L_II^-1 (E_I - sum of the row's partial tiles in chunk order), one workgroup per
//                     (row I, block of 64 columns); one launch per level
//   k_fsol_bsolve     the same two with L^T, the backward pass of the multi-RHS solve (k_factorsolve.hip launches
//   k_fsol_bepilogue  it): partial tile sum_{I in chunk} L_IJ^T X_I per (column J, chunk, block of 64 columns), and
//                     X_J = L_JJ^-T (D_J Y_J - the column's partial tiles in chunk order).  L_IJ is then read as it
//                     lies in memory, rows = k: it is the k-major operand, and linvT[J] = L_JJ^-T the index-major one
//   k_joint_gram      partial tile sum_{I in group} Y_I^T D_I Y_I, one workgroup per (group of <= 8 reach rows,
//                     lower 64 x 64 tile of the output)
//   k_joint_combine   the groups summed in order, the lower half mirrored into the upper one
//   k_joint_lmdiag    V_l^-1 added to the diagonal block of every requested landmark, both halves from the lower one
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
#include "jointstate.h"
#include "lm_entry.h"
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

// The substitution with L (T = false: forward, rows I, sources J < I) or with L^T (T = true: the backward pass of
// the multi-RHS solve, columns J, sources I > J; k_factorsolve.hip launches it).  Panel of tile t: pos[t]; the
// transposed pass visits every tile row, its panel t is tile t and it has no pos.
// chunks: (R, position of R, first source, end source) of one level, R the row (column) being solved; slot
// (blockIdx.x, blockIdx.y) = the partial tile sum_{S in chunk} L_RS Y_S (L_SR^T Y_S) of columns [64 b, 64 b + 64)
template <bool T>
__device__ __forceinline__ void subst_partial(Lds& s, const uint4* __restrict__ chunks, const uint32_t* __restrict__ src,
                                              const uint32_t* __restrict__ pos, const double* __restrict__ A, uint32_t ld,
                                              const double* __restrict__ Y, uint32_t mp, double* __restrict__ slots) {
  const uint4 c = chunks[blockIdx.x];
  const uint32_t R = c.x, s0 = c.z, b = blockIdx.y;
  double4_t acc[2][2];
  zero_acc(acc);
  Chunk ca, cb;
  auto fetch = [&](uint32_t ch) {
    const uint32_t S = src[s0 + (ch >> 1)];
    const int k0 = KCH * (int)(ch & 1);
    uint32_t panel = S;
    if constexpr (T) {
      load_kmajor(ca, A + (size_t)S * TB * ld + (size_t)R * TB, ld, k0);   // X[k][r] = L_SR[k][r], as it lies
    } else {
      load_imajor(ca, A + (size_t)R * TB * ld + (size_t)S * TB, ld, k0);   // X[k][r] = L_RS[r][k]
      panel = pos[S];
    }
    load_kmajor(cb, Y + (size_t)panel * TB * mp + (size_t)b * TB, mp, k0);   // Y[k][x] = Y_S[k][x]
  };
  accumulate_chunks(acc, s, 2 * (c.w - s0), fetch, [&](uint32_t) {
    if constexpr (T) store_kmajor(ca, s.X);
    else store_imajor(ca, s.X);
    store_kmajor(cb, s.Y);
  });
  store_tile(slots + ((size_t)blockIdx.x * gridDim.y + b) * (TB * TB), TB, acc);
}

// rows: (R, first chunk, end chunk, first chunk of the level) of one level.
// Y_R = G V with V = Y_R (T: D_R Y_R, the sign of row k going on while Y_R is read) - the row's partial tiles in
// chunk order, and G = L_RR^-1, linvT[R] read k-major (T: L_RR^-T, linvT[R] read index-major).  The sign is a
// compile-time choice: a run-time test would put a branch around each of the 16 first loads.
template <bool T>
__device__ __forceinline__ void subst_epilogue(Lds& s, const uint4* __restrict__ rows, const uint32_t* __restrict__ pos,
                                               const double* __restrict__ linvT, const double* __restrict__ dsgn,
                                               double* __restrict__ Y, uint32_t mp, const double* __restrict__ slots) {
  const uint4 r = rows[blockIdx.x];
  const uint32_t R = r.x, b = blockIdx.y, ncb = gridDim.y;
  uint32_t panel = R;
  if constexpr (!T) panel = pos[R];
  double* YR = Y + (size_t)panel * TB * mp + (size_t)b * TB;
  const double* G = linvT + (size_t)R * TB * TB;  // linvT[R][c][x] = (L_RR^-1)[x][c]
  const int tid = threadIdx.x;
  // V first, both 32-row halves at once.  Thread t owns elements e = t + 256 q of the 64 x 64 tile; each element
  // subtracts its slots in chunk order
  double v[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int k = (tid + 256 * q) / TB;
    v[q] = YR[(size_t)k * mp + tid % TB];
    if constexpr (T) v[q] *= dsgn[(size_t)R * TB + k];
  }
  const double* sl = slots + ((size_t)(r.y - r.w) * ncb + b) * (TB * TB) + tid;
  for (uint32_t c = r.y; c < r.z; ++c, sl += (size_t)ncb * (TB * TB)) {
    double w[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) w[q] = sl[256 * q];
    // The 16 loads of a slot are independent and must be in flight together.  Without the barrier the compiler pulls
    // the first two adds, and the wait they need, in front of the other fourteen loads: a memory round trip more per
    // slot, 24 % of the substitution where a row has 50 slots.
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] -= w[q];
  }
  double4_t out[2][2];
  zero_acc(out);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    Chunk cg;
    if constexpr (T) {
      load_imajor(cg, G, TB, KCH * h);
      store_imajor(cg, s.X);
    } else {
      load_kmajor(cg, G, TB, KCH * h);
      store_kmajor(cg, s.X);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) s.Y[(tid + 256 * q) / TB][tid % TB] = v[8 * h + q];
    __syncthreads();
    mma_chunk(out, s);
    __syncthreads();
  }
  store_tile(YR, mp, out);
}

__global__ void __launch_bounds__(256)
k_joint_fsolve(const uint4* __restrict__ chunks, const uint32_t* __restrict__ src, const uint32_t* __restrict__ pos,
               const double* __restrict__ A, uint32_t ld, const double* __restrict__ Y, uint32_t mp,
               double* __restrict__ slots) {
  __shared__ Lds s;
  subst_partial<false>(s, chunks, src, pos, A, ld, Y, mp, slots);
}
__global__ void __launch_bounds__(256)
k_joint_epilogue(const uint4* __restrict__ rows, const uint32_t* __restrict__ pos, const double* __restrict__ linvT,
                 double* __restrict__ Y, uint32_t mp, const double* __restrict__ slots) {
  __shared__ Lds s;
  subst_epilogue<false>(s, rows, pos, linvT, nullptr, Y, mp, slots);
}
__global__ void __launch_bounds__(256)
k_fsol_bsolve(const uint4* __restrict__ chunks, const uint32_t* __restrict__ src, const double* __restrict__ A, uint32_t ld,
              const double* __restrict__ X, uint32_t mp, double* __restrict__ slots) {
  __shared__ Lds s;
  subst_partial<true>(s, chunks, src, nullptr, A, ld, X, mp, slots);
}
__global__ void __launch_bounds__(256)
k_fsol_bepilogue(const uint4* __restrict__ rows, const double* __restrict__ linvT, const double* __restrict__ dsgn,
                 double* __restrict__ X, uint32_t mp, const double* __restrict__ slots) {
  __shared__ Lds s;
  subst_epilogue<true>(s, rows, nullptr, linvT, dsgn, X, mp, slots);
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
  accumulate_chunks(acc, s, 2 * (q1 - q0), fetch, [&](uint32_t) {
    store_kmajor(ca, s.X);
    store_kmajor(cb, s.Y);
  });
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

// ---- landmark columns (jointstate.h; LmArgs, lm_entry: lm_entry.h) -----------------------------------------
// does landmark l (LM == 1) have an observation from a pose other than its reference pose?  All 64 lanes call.
template <int LM>
__device__ __forceinline__ bool joint_any_listed(const LmArgs& g, uint32_t l, uint32_t nobs, int lane) {
  bool any_listed = false;
  if (LM == 1) {
    const uint32_t rp = g.lm_ref_pose[l];
    for (uint32_t e0 = 0; e0 < nobs; e0 += 64) {
      const uint32_t e = e0 + lane;
      const bool lst = e < nobs && g.obs_pose[g.lm_ptr[l] + e] != rp;
      any_listed = any_listed || __ballot(lst) != 0;
    }
  }
  return any_listed;
}
// a landmark without observations has no incidence (its E_l is zero)
template <int LM>
__device__ __forceinline__ uint32_t joint_entries(const LmArgs& g, uint32_t nobs) {
  return nobs ? nobs + (LM == 1 ? 1u : 0u) + (g.K > 0 ? 1u : 0u) : 0u;
}

// marks[t] = 1 for every tile row t (< nt) that a valid incidence of a requested landmark touches (zeroed by the
// caller; every writer stores the same word), cnt[q] = the valid incidences of ids[q]
template <int LM>
__global__ void __launch_bounds__(256)
k_joint_seed(LmArgs g, uint32_t n, const uint32_t* __restrict__ ids, uint32_t* __restrict__ marks,
             uint32_t* __restrict__ cnt) {
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n) return;
  const int lane = threadIdx.x & 63;
  const uint32_t l = ids[q], nobs = g.lm_ptr[l + 1] - g.lm_ptr[l];
  const bool any_listed = joint_any_listed<LM>(g, l, nobs, lane);
  const uint32_t ne = joint_entries<LM>(g, nobs);
  uint32_t c = 0;
  for (uint32_t e = lane; e < ne; e += 64) {
    const LmEntry<LM> x = lm_entry<LM>(g, l, e, nobs, any_listed);
    if (!x.valid) continue;
    ++c;
    const uint32_t t0 = x.base / TB, t1 = (x.base + (uint32_t)x.width - 1) / TB;   // a block may straddle two tiles
    if (t0 < g.nt) marks[t0] = 1;
    if (t1 < g.nt) marks[t1] = 1;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
  if (lane == 0) cnt[q] = c;
}

// Column c0 + LM q + k of landmark ids[q]: lane i LM + k owns entry (i, k) of every incidence and adds
// -(W_e V^-1)[i][k] into row base + i of the panel that holds it.  One lane, one column, incidences in order: the
// sums do not depend on the launch or on the other columns.
template <int LM>
__global__ void __launch_bounds__(256)
k_joint_rhs(LmArgs g, uint32_t n, const uint32_t* __restrict__ ids, uint32_t c0, const uint32_t* __restrict__ pos,
            double* __restrict__ Y, uint32_t mp) {
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n) return;
  const int lane = threadIdx.x & 63;
  const uint32_t l = ids[q], nobs = g.lm_ptr[l + 1] - g.lm_ptr[l];
  const bool any_listed = joint_any_listed<LM>(g, l, nobs, lane);
  const uint32_t ne = joint_entries<LM>(g, nobs);
  double Vi[LM * LM];
  joint_lm_vinv<LM>(nobs, g.lm_vinv + (size_t)l * LM * LM, Vi);
  const int i = lane / LM, k = lane % LM;
  if (i >= 6) return;
  for (uint32_t e = 0; e < ne; ++e) {
    const LmEntry<LM> x = lm_entry<LM>(g, l, e, nobs, any_listed);
    if (!x.valid || i >= x.width) continue;
    const uint32_t row = x.base + (uint32_t)i, t = row / TB;
    const uint32_t pq = t < g.nt ? pos[t] : kJointNone;
    if (pq == kJointNone) continue;   // (k_joint_seed marked the tile: it is in the reach)
    Y[((size_t)pq * TB + row % TB) * mp + c0 + (uint32_t)LM * q + (uint32_t)k] += joint_lm_value<LM>(x.w, Vi, i, k);
  }
}

// out[c0 + LM q + a][c0 + LM q + b] += V^-1[a][b] for b <= a, mirrored (out stays bitwise symmetric)
template <int LM>
__global__ void __launch_bounds__(256)
k_joint_lmdiag(const uint32_t* __restrict__ lm_ptr, const double* __restrict__ lm_vinv, uint32_t n,
               const uint32_t* __restrict__ ids, uint32_t c0, uint32_t M, double* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * LM * LM) return;
  const uint32_t q = t / (LM * LM), a = (t / LM) % LM, b = t % LM;
  if (b > a) return;
  const uint32_t l = ids[q];
  double Vi[LM * LM];
  joint_lm_vinv<LM>(lm_ptr[l + 1] - lm_ptr[l], lm_vinv + (size_t)l * LM * LM, Vi);
  const size_t r = c0 + (size_t)LM * q + a, c = c0 + (size_t)LM * q + b;
  const double s = out[r * M + c] + Vi[a * LM + b];
  out[r * M + c] = s;
  out[c * M + r] = s;
}

// ---- host side ----------------------------------------------------------------------------------------
// The substitution over the levels of a plan, two launches per level (engine.h): Y <- L^-1 Y over the plan's reach
// (dsgn unused), or with `transposed` the backward pass Y <- L^-T D Y of the multi-RHS solve in k_factorsolve.hip,
// whose plan holds every tile row.
void joint_subst_launch(hipStream_t stream, const JointPlan& p, const SubstTables& t, bool transposed, const double* A,
                        uint32_t ld, const double* linvT, const double* dsgn, double* Y, double* slots) {
  const uint32_t mp = p.m_pad, ncb = p.ncb;
  for (uint32_t v = 0; v < p.levels(); ++v) {
    const uint32_t c0 = p.chunk_level_ptr[v], c1 = p.chunk_level_ptr[v + 1];
    if (c1 > c0 && transposed)
      hipLaunchKernelGGL(k_fsol_bsolve, dim3(c1 - c0, ncb), dim3(256), 0, stream, t.chunks + c0, t.src, A, ld,
                         (const double*)Y, mp, slots);
    else if (c1 > c0)
      hipLaunchKernelGGL(k_joint_fsolve, dim3(c1 - c0, ncb), dim3(256), 0, stream, t.chunks + c0, t.src, t.pos, A, ld,
                         (const double*)Y, mp, slots);
    const uint32_t r0 = p.level_ptr[v], r1 = p.level_ptr[v + 1];
    if (transposed)
      hipLaunchKernelGGL(k_fsol_bepilogue, dim3(r1 - r0, ncb), dim3(256), 0, stream, t.rows + r0, linvT, dsgn, Y, mp,
                         (const double*)slots);
    else
      hipLaunchKernelGGL(k_joint_epilogue, dim3(r1 - r0, ncb), dim3(256), 0, stream, t.rows + r0, t.pos, linvT, Y, mp,
                         (const double*)slots);
  }
}

// sel: the requested rows of S in the engine's (factorised) numbering (unit columns), lms: the requested landmarks
// (active, checked by the caller), whose LM columns each follow those of sel; out: M x M on the host
int jointcov_run(Engine* e, const std::vector<uint32_t>& sel, const std::vector<uint32_t>& lms, double* out) {
  const Structure& st = e->st;
  const int LM = e->lm_dim;
  const uint32_t Ms = (uint32_t)sel.size(), nl = (uint32_t)lms.size(), M = Ms + nl * (uint32_t)LM;
  uint32_t nt;
  const double *dsgn, *linvT;
  if (int rc = kept_factor(e, "joint marginals", &nt, &dsgn, &linvT)) return rc;
  std::vector<uint32_t> tiles(Ms);
  for (uint32_t c = 0; c < Ms; ++c) tiles[c] = sel[c] / TB;
  // the landmark columns: ids | marks (nt) | incidence counts, the tile rows they touch from the device
  ba_hip_joint_state_stats ss = {};
  LmArgs g = {};
  const uint32_t* d_ids = nullptr;
  if (nl) {
    g = lm_args(e);
    if (e->jc_lm.alloc(2 * (size_t)nl + nt) != hipSuccess) {
      (void)hipGetLastError();
      jointcov_release(e);
      char msg[160];
      snprintf(msg, sizeof msg, "joint marginals: allocating the landmark tables (%zu bytes, %u landmarks) failed",
               (2 * (size_t)nl + nt) * sizeof(uint32_t), nl);
      return e->fail_msg(msg);
    }
    uint32_t* d_marks = e->jc_lm.p + nl;
    d_ids = e->jc_lm.p;
    BAE_HIP(hipMemcpyAsync(e->jc_lm.p, lms.data(), nl * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    BAE_HIP(hipMemsetAsync(d_marks, 0, ((size_t)nt + nl) * sizeof(uint32_t), e->stream));
    Events<2> evs;
    BAE_HIP(evs.create());
    (void)evs.record(0, e->stream);
    if (LM == 1) hipLaunchKernelGGL(k_joint_seed<1>, dim3((nl + 3) / 4), dim3(256), 0, e->stream, g, nl, d_ids, d_marks, d_marks + nt);
    else hipLaunchKernelGGL(k_joint_seed<3>, dim3((nl + 3) / 4), dim3(256), 0, e->stream, g, nl, d_ids, d_marks, d_marks + nt);
    (void)evs.record(1, e->stream);
    const hipError_t lerr = hipGetLastError();
    if (lerr != hipSuccess) return e->fail(lerr, "k_joint_seed launch");
    std::vector<uint32_t> marks((size_t)nt + nl);
    BAE_HIP(hipMemcpyAsync(marks.data(), d_marks, marks.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    BAE_HIP(hipStreamSynchronize(e->stream));
    ss.seed_ms = evs.ms(0, 1);
    for (uint32_t t = 0; t < nt; ++t)
      if (marks[t]) { tiles.push_back(t); ++ss.seed_tiles; }
    for (uint32_t q = 0; q < nl; ++q) ss.incidences += marks[nt + q];
    ss.landmark_columns = nl * (uint32_t)LM;
  }
  JointPlan p;
  build_joint_plan(e->nzL_host, nt, tiles, M, p);
  const uint32_t nr = (uint32_t)p.reach.size(), mp = p.m_pad, ncb = p.ncb, ntl = ncb * (ncb + 1) / 2;
  std::vector<uint32_t> key(mp, kJointNone);
  for (uint32_t c = 0; c < Ms; ++c) key[c] = p.pos[sel[c] / TB] * TB + sel[c] % TB;
  IndexPack idx;   // one index buffer
  const size_t o_chunks = idx.add(p.chunks, 4), o_rows = idx.add(p.rows, 4), o_src = idx.add(p.src), o_pos = idx.add(p.pos),
               o_reach = idx.add(p.reach), o_key = idx.add(key);
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
  BAE_HIP(idx.upload(e->jc_idx));
  const SubstTables tab = {idx.at<uint4>(o_chunks), idx.at<uint4>(o_rows), idx.at(o_src), idx.at(o_pos)};
  Events<5> ev;   // start, substitution done, end; around the right-hand-side pass
  BAE_HIP(ev.create());
  (void)ev.record(0, e->stream);
  // (a request whose columns are all zero has an empty reach: nothing to initialise, solve or multiply)
  if (n_y)
    hipLaunchKernelGGL(k_joint_init, dim3((unsigned)((n_y + 255) / 256)), dim3(256), 0, e->stream, e->jc_Y.p, (uint64_t)n_y,
                       mp, idx.at(o_key));
  const bool rhs = nl && nr;
  if (rhs) {
    (void)ev.record(3, e->stream);
    if (LM == 1) hipLaunchKernelGGL(k_joint_rhs<1>, dim3((nl + 3) / 4), dim3(256), 0, e->stream, g, nl, d_ids, Ms, tab.pos, e->jc_Y.p, mp);
    else hipLaunchKernelGGL(k_joint_rhs<3>, dim3((nl + 3) / 4), dim3(256), 0, e->stream, g, nl, d_ids, Ms, tab.pos, e->jc_Y.p, mp);
    (void)ev.record(4, e->stream);
  }
  joint_subst_launch(e->stream, p, tab, false, e->A.p, st.ld, linvT, nullptr, e->jc_Y.p, e->jc_slots.p);
  (void)ev.record(1, e->stream);
  if (p.gram_groups)
    hipLaunchKernelGGL(k_joint_gram, dim3(p.gram_groups, ntl), dim3(256), 0, e->stream, (const double*)e->jc_Y.p, mp,
                       idx.at(o_reach), nr, dsgn, e->jc_part.p);
  hipLaunchKernelGGL(k_joint_combine, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, e->stream,
                     (const double*)e->jc_part.p, p.gram_groups, ntl, M, e->jc_out.p);
  if (nl) {
    const unsigned nb = (nl * (uint32_t)(LM * LM) + 255) / 256;
    if (LM == 1) hipLaunchKernelGGL(k_joint_lmdiag<1>, dim3(nb), dim3(256), 0, e->stream, g.lm_ptr, g.lm_vinv, nl, d_ids, Ms, M, e->jc_out.p);
    else hipLaunchKernelGGL(k_joint_lmdiag<3>, dim3(nb), dim3(256), 0, e->stream, g.lm_ptr, g.lm_vinv, nl, d_ids, Ms, M, e->jc_out.p);
  }
  (void)ev.record(2, e->stream);
  const hipError_t lerr = hipGetLastError();
  const hipError_t serr = hipEventSynchronize(ev[2]);
  ba_hip_joint_marginal_stats js = {};
  if (rhs) ss.rhs_ms = ev.ms(3, 4);
  js.solve_ms = ev.ms(0, 1) - ss.rhs_ms;
  js.gram_ms = ev.ms(1, 2);
  if (lerr != hipSuccess) return e->fail(lerr, "k_joint launch");
  if (serr != hipSuccess) return e->fail(serr, "k_joint");
  BAE_HIP(hipMemcpy(out, e->jc_out.p, n_out * sizeof(double), hipMemcpyDeviceToHost));
  js.columns = M;
  js.reach_tiles = nr;
  js.levels = p.levels();
  js.tile_products = p.products;
  js.workspace_bytes = (double)(e->jc_idx.bytes() + e->jc_Y.bytes() + e->jc_slots.bytes() + e->jc_part.bytes() +
                                e->jc_out.bytes() + e->jc_lm.bytes());
  e->jstats = js;
  if (nl) e->jsstats = ss;
  return 0;
}

void jointcov_release(Engine* e) {   // (ba_hip_release_marginals promises the memory back while the engine lives)
  e->jc_idx.release(); e->jc_Y.release(); e->jc_slots.release(); e->jc_part.release(); e->jc_out.release(); e->jc_lm.release();
}

}  // namespace bae
