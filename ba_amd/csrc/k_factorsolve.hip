// Solves with the factor that ba_hip_solve_gn leaves behind (ba_hip_factor_solve): X = S^-1 B for a caller's block
// of m <= 512 right-hand sides, S = L D L^T tile-sparse.  One 64 x m_pad panel per tile row, solved in place by the
// substitution of k_jointcov.hip (joint_subst_launch) seeded with every tile row: the forward pass Y = L^-1 B
// (k_joint_fsolve / k_joint_epilogue), then its mirror on the mirrored plan, the backward pass
// X_J = L_JJ^-T (D_J Y_J - sum_{I > J} L_IJ^T X_I) (k_fsol_bsolve / k_fsol_bepilogue, also there).  Here are
//
//   k_panel_scatter   B (n x m, the caller's row order) -> panels in the factorised row order, zeros in padding rows
//                     and padding columns (also the panels of k_pcg_panel.hip)
//   k_panel_gather    panels -> X (n x m, the caller's row order)
//
// and the weakest modes of S (ba_hip_get_weakest_modes): the block inverse iteration of factorsolve.h on three
// panels of 64 columns that stay on the device, S^-1 applied by the kernels above, the 64 x 64 matrices on the host:
//
//   k_mode_gram       partial tile sum_{t in group} X_t^T Y_t of two panels, one workgroup per group of <= 8 tile rows
//   k_mode_combine    the groups summed in order
//   k_mode_apply      X_t <- X_t M for a 64 x 64 M, one workgroup per tile row, in place
//   k_mode_residual   R = W - Q diag(theta), element by element
//
// The plan (levels, chunks, slots of both passes) and the host restatement are in factorsolve.h, checked on the
// CPU by tests/test_factor_solve_plan.py.  The factor is read, never written: L_IJ from A, L_JJ^-T (linvT) and the
// pivot signs D from invdiag.  FP64, no atomics: every partial tile and every panel element has one writer and the
// sums run in the plan's order, so two calls give the same bits.
//
// The tile products run on v_mfma_f64_16x16x4_f64 with the staging of tile_mma.h, as in k_jointcov.hip.
#include "engine.h"
#include "factorsolve.h"
#include "tile_mma.h"

#include <algorithm>
#include <chrono>
#include <vector>

namespace bae {

using namespace tile64;

// rowmap[i]: the caller's row of panel row i (kJointNone for a padding row), i < count / mp
__global__ void __launch_bounds__(256)
k_panel_scatter(const double* __restrict__ B, uint32_t m, const uint32_t* __restrict__ rowmap, uint64_t count, uint32_t mp,
                double* __restrict__ X) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const uint32_t c = (uint32_t)(t % mp), r = rowmap[t / mp];
  X[t] = (c < m && r != kJointNone) ? B[(size_t)r * m + c] : 0.0;
}

__global__ void __launch_bounds__(256)
k_panel_gather(const double* __restrict__ X, uint32_t mp, const uint32_t* __restrict__ rowmap, uint64_t count, uint32_t m,
               double* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const uint32_t c = (uint32_t)(t % mp), r = rowmap[t / mp];
  if (c < m && r != kJointNone) out[(size_t)r * m + c] = X[t];
}

void panel_scatter_launch(hipStream_t stream, const double* B, uint32_t m, const uint32_t* rowmap, uint64_t count,
                          uint32_t mp, double* X) {
  hipLaunchKernelGGL(k_panel_scatter, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, B, m, rowmap, count, mp, X);
}
void panel_gather_launch(hipStream_t stream, const double* X, uint32_t mp, const uint32_t* rowmap, uint64_t count,
                         uint32_t m, double* out) {
  hipLaunchKernelGGL(k_panel_gather, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, X, mp, rowmap, count, m, out);
}

// part[g] = sum_{t in group g} X_t^T Y_t: both panels are k-major operands as they lie (rows = k)
__global__ void __launch_bounds__(256)
k_mode_gram(const double* __restrict__ X, const double* __restrict__ Y, uint32_t nt, double* __restrict__ part) {
  __shared__ Lds s;
  const uint32_t g = blockIdx.x;
  const uint32_t t0 = g * kModeGramGroup, t1 = min(nt, t0 + kModeGramGroup);
  double4_t acc[2][2];
  zero_acc(acc);
  Chunk ca, cb;
  auto fetch = [&](uint32_t ch) {
    const size_t off = (size_t)(t0 + (ch >> 1)) * TB * kModeBlock;
    const int k0 = KCH * (int)(ch & 1);
    load_kmajor(ca, X + off, kModeBlock, k0);
    load_kmajor(cb, Y + off, kModeBlock, k0);
  };
  accumulate_chunks(acc, s, 2 * (t1 - t0), fetch, [&](uint32_t) {
    store_kmajor(ca, s.X);
    store_kmajor(cb, s.Y);
  });
  store_tile(part + (size_t)g * (TB * TB), TB, acc);
}

__global__ void __launch_bounds__(256)
k_mode_combine(const double* __restrict__ part, uint32_t groups, double* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;   // < 64 * 64: the launch is 16 x 256
  double sum = 0.0;
  for (uint32_t g = 0; g < groups; ++g) sum += part[(size_t)g * (TB * TB) + t];
  out[t] = sum;
}

// X_t <- X_t M.  The tile row is read into registers whole before anything is written: X_t is the index-major operand
__global__ void __launch_bounds__(256)
k_mode_apply(double* __restrict__ X, const double* __restrict__ M) {
  __shared__ Lds s;
  double* Xt = X + (size_t)blockIdx.x * TB * kModeBlock;
  Chunk ca[2], cb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    load_imajor(ca[h], Xt, kModeBlock, KCH * h);   // X[k][i] = X_t[i][k]
    load_kmajor(cb[h], M, TB, KCH * h);            // Y[k][j] = M[k][j]
  }
  double4_t acc[2][2];
  zero_acc(acc);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    store_imajor(ca[h], s.X);
    store_kmajor(cb[h], s.Y);
    __syncthreads();
    mma_chunk(acc, s);
    __syncthreads();
  }
  store_tile(Xt, kModeBlock, acc);
}

__global__ void __launch_bounds__(256)
k_mode_residual(const double* __restrict__ W, const double* __restrict__ Q, const double* __restrict__ theta, uint64_t count,
                double* __restrict__ R) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  R[t] = W[t] - Q[t] * theta[t % kModeBlock];
}

// ---- host side ----------------------------------------------------------------------------------------
namespace {

// the plan's tables on the device, one buffer; pos is the identity and serves both passes
struct FsolTables {
  SubstTables fwd, bwd;
  const uint32_t* rowmap;
};

int fsol_prepare(Engine* e, const FactorRef& f, const uint32_t* rowmap, const FactorSolvePlan& p, size_t n_stage,
                 FsolTables* t, uint32_t panels = 1) {
  const JointPlan &pf = p.fwd, &pb = p.bwd;
  const uint32_t nt = f.nt, rows = nt * (uint32_t)TB;
  IndexPack idx;
  const size_t o_fc = idx.add(pf.chunks, 4), o_fr = idx.add(pf.rows, 4), o_bc = idx.add(pb.chunks, 4), o_br = idx.add(pb.rows, 4),
               o_fs = idx.add(pf.src), o_bs = idx.add(pb.src), o_pos = idx.add(pf.pos), o_map = idx.add(rowmap, rowmap + rows);
  const size_t n_x = panels * pf.y_count(), n_slots = (size_t)std::max(p.max_level_chunks(), 1u) * pf.ncb * TB * TB;
  if (e->fs_idx.alloc(idx.size()) != hipSuccess || e->fs_X.alloc(n_x) != hipSuccess ||
      e->fs_slots.alloc(n_slots) != hipSuccess || e->fs_B.alloc(n_stage) != hipSuccess) {
    (void)hipGetLastError();
    factor_solve_release(e);
    char msg[160];
    snprintf(msg, sizeof msg, "factor solve: allocating the workspace (%zu bytes, %u tiles, %u columns) failed",
             (n_x + n_slots + n_stage) * sizeof(double) + idx.size() * sizeof(uint32_t), nt, pf.m);
    return e->fail_msg(msg);
  }
  BAE_HIP(idx.upload(e->fs_idx));
  t->fwd = {idx.at<uint4>(o_fc), idx.at<uint4>(o_fr), idx.at(o_fs), idx.at(o_pos)};
  t->bwd = {idx.at<uint4>(o_bc), idx.at<uint4>(o_br), idx.at(o_bs), idx.at(o_pos)};
  t->rowmap = idx.at(o_map);
  return 0;
}

// X <- S^-1 X on the panels, enqueued on e->stream; ev (optional): events 1 and 2 after the two passes
void fsol_apply(Engine* e, const FactorRef& f, const FactorSolvePlan& p, const FsolTables& t, double* X, Events<4>* ev) {
  joint_subst_launch(e->stream, p.fwd, t.fwd, false, f.A, f.ld, f.linvT, nullptr, X, e->fs_slots.p);
  if (ev) (void)ev->record(1, e->stream);
  joint_subst_launch(e->stream, p.bwd, t.bwd, true, f.A, f.ld, f.linvT, f.dsgn, X, e->fs_slots.p);
  if (ev) (void)ev->record(2, e->stream);
}

}  // namespace

int factor_solve_run(Engine* e, const FactorRef& f, uint32_t n, const uint32_t* rowmap, uint32_t m, const double* B,
                     double* X) {
  FactorSolvePlan p;
  build_factor_solve_plan(*f.nz, f.nt, m, p);
  FsolTables t;
  const size_t n_io = (size_t)n * m;
  if (int rc = fsol_prepare(e, f, rowmap, p, n_io, &t)) return rc;
  const uint32_t mp = p.fwd.m_pad;
  const uint64_t n_x = p.fwd.y_count();
  BAE_HIP(hipMemcpyAsync(e->fs_B.p, B, n_io * sizeof(double), hipMemcpyHostToDevice, e->stream));
  Events<4> ev;   // start, forward done, backward done, end
  BAE_HIP(ev.create());
  panel_scatter_launch(e->stream, e->fs_B.p, m, t.rowmap, n_x, mp, e->fs_X.p);
  (void)ev.record(0, e->stream);
  fsol_apply(e, f, p, t, e->fs_X.p, &ev);
  panel_gather_launch(e->stream, e->fs_X.p, mp, t.rowmap, n_x, m, e->fs_B.p);
  (void)ev.record(3, e->stream);
  const hipError_t lerr = hipGetLastError();
  const hipError_t serr = hipEventSynchronize(ev[3]);
  if (lerr != hipSuccess) return e->fail(lerr, "k_fsol launch");
  if (serr != hipSuccess) return e->fail(serr, "k_fsol");
  BAE_HIP(hipMemcpy(X, e->fs_B.p, n_io * sizeof(double), hipMemcpyDeviceToHost));
  ba_hip_factor_solve_stats s = {};
  s.forward_ms = ev.ms(0, 1);
  s.backward_ms = ev.ms(1, 2);
  s.workspace_bytes = (double)(e->fs_idx.bytes() + e->fs_X.bytes() + e->fs_slots.bytes() + e->fs_B.bytes());
  s.tile_products = p.products();
  s.columns = m;
  s.tiles = f.nt;
  s.forward_levels = p.fwd.levels();
  s.backward_levels = p.bwd.levels();
  e->fsstats = s;
  return 0;
}

namespace {

// the Ops of weakest_modes_iterate (factorsolve.h) on the device: panels 0, 1, 2 in fs_X, M and theta in fs_M, the
// partial Gram tiles and their sum in fs_part.  Every host matrix goes up and comes down through e->stream, which is
// drained on the spot: the host buffers are reused by the caller.  The first HIP error is kept and ends the work.
struct DeviceModeOps {
  Engine* e;
  const FactorRef& f;
  const FactorSolvePlan& p;
  const FsolTables& t;
  uint32_t n;
  const uint32_t* rowmap;   // host
  size_t panel;             // doubles per panel
  uint32_t groups;
  hipError_t err = hipSuccess;
  double solve_ms = 0.0, ortho_ms = 0.0;
  std::chrono::steady_clock::time_point t0;
  double* P(int a) const { return e->fs_X.p + (size_t)a * panel; }
  void keep(hipError_t x) { if (err == hipSuccess) err = x; }
  void drain() { keep(hipGetLastError()); keep(hipStreamSynchronize(e->stream)); }
  void start(int a, uint32_t seed, uint32_t pcols) {
    std::vector<double> B((size_t)n * kModeBlock, 0.0);
    for (uint32_t r = 0; r < n; ++r)
      for (uint32_t c = 0; c < pcols; ++c) B[(size_t)r * kModeBlock + c] = mode_start_value(seed, r, c);
    if (err != hipSuccess) return;
    keep(hipMemcpyAsync(e->fs_B.p, B.data(), B.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    panel_scatter_launch(e->stream, e->fs_B.p, kModeBlock, t.rowmap, (uint64_t)panel, kModeBlock, P(a));
    drain();
  }
  void gram(int a, int b, double* G) {
    if (err != hipSuccess) { std::fill(G, G + TB * TB, 0.0); return; }
    double* out = e->fs_part.p + (size_t)groups * (TB * TB);
    hipLaunchKernelGGL(k_mode_gram, dim3(groups), dim3(256), 0, e->stream, (const double*)P(a), (const double*)P(b), f.nt,
                       e->fs_part.p);
    hipLaunchKernelGGL(k_mode_combine, dim3(TB * TB / 256), dim3(256), 0, e->stream, (const double*)e->fs_part.p, groups, out);
    keep(hipMemcpyAsync(G, out, TB * TB * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    drain();
  }
  void apply(int a, const double* M) {
    if (err != hipSuccess) return;
    keep(hipMemcpyAsync(e->fs_M.p, M, TB * TB * sizeof(double), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_mode_apply, dim3(f.nt), dim3(256), 0, e->stream, P(a), (const double*)e->fs_M.p);
    drain();
  }
  void copy(int dst, int src) {
    if (err != hipSuccess) return;
    keep(hipMemcpyAsync(P(dst), P(src), panel * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  }
  void solve(int a) {
    if (err != hipSuccess) return;
    fsol_apply(e, f, p, t, P(a), nullptr);
  }
  void residual(int w, int q, const double* theta, int r) {
    if (err != hipSuccess) return;
    double* d_theta = e->fs_M.p + TB * TB;
    keep(hipMemcpyAsync(d_theta, theta, kModeBlock * sizeof(double), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_mode_residual, dim3((unsigned)((panel + 255) / 256)), dim3(256), 0, e->stream, (const double*)P(w),
                       (const double*)P(q), (const double*)d_theta, (uint64_t)panel, P(r));
    drain();
  }
  double since() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
  void svqb_begin() { t0 = std::chrono::steady_clock::now(); }
  void svqb_end() { ortho_ms += since(); }
  void solve_begin() { t0 = std::chrono::steady_clock::now(); }
  void solve_end() { drain(); solve_ms += since(); }
};

}  // namespace

int weakest_modes_run(Engine* e, const FactorRef& f, uint32_t n, const uint32_t* rowmap, uint32_t k, const ModeOptions& o,
                      double* eigenvalues, double* modes) {
  FactorSolvePlan p;
  build_factor_solve_plan(*f.nz, f.nt, kModeBlock, p);
  FsolTables t;
  const size_t n_io = (size_t)n * kModeBlock;
  if (int rc = fsol_prepare(e, f, rowmap, p, n_io, &t, 3)) return rc;
  const uint32_t groups = (f.nt + kModeGramGroup - 1) / kModeGramGroup;
  if (e->fs_M.alloc(TB * TB + kModeBlock) != hipSuccess || e->fs_part.alloc((size_t)(groups + 1) * TB * TB) != hipSuccess) {
    (void)hipGetLastError();
    factor_solve_release(e);
    char msg[160];
    snprintf(msg, sizeof msg, "weakest modes: allocating the Gram workspace (%zu bytes, %u tiles) failed",
             ((size_t)(groups + 2) * TB * TB + kModeBlock) * sizeof(double), f.nt);
    return e->fail_msg(msg);
  }
  DeviceModeOps ops = {e, f, p, t, n, rowmap, p.fwd.y_count(), groups};
  ModeResult r;
  weakest_modes_iterate(ops, n, k, o, r);
  if (ops.err != hipSuccess) return e->fail(ops.err, "k_mode");
  panel_gather_launch(e->stream, ops.P(r.panel), kModeBlock, t.rowmap, (uint64_t)ops.panel, kModeBlock, e->fs_B.p);
  std::vector<double> Qv(n_io);
  BAE_HIP(hipGetLastError());
  BAE_HIP(hipMemcpyAsync(Qv.data(), e->fs_B.p, n_io * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  BAE_HIP(hipStreamSynchronize(e->stream));
  modes_finish(r, n, k, Qv.data(), eigenvalues, modes);
  ba_hip_mode_stats s = {};
  s.solve_ms = ops.solve_ms;
  s.ortho_ms = ops.ortho_ms;
  s.residual_max = r.residual_max;
  s.workspace_bytes = (double)(e->fs_idx.bytes() + e->fs_X.bytes() + e->fs_slots.bytes() + e->fs_B.bytes() +
                               e->fs_M.bytes() + e->fs_part.bytes());
  s.iterations = r.iterations;
  s.converged = r.converged;
  s.block = r.block;
  e->mode_stats = s;
  return 0;
}

void factor_solve_release(Engine* e) {   // (ba_hip_release_marginals promises the memory back while the engine lives)
  e->fs_idx.release(); e->fs_X.release(); e->fs_slots.release(); e->fs_B.release(); e->fs_M.release(); e->fs_part.release();
}

}  // namespace bae
