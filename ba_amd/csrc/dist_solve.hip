// Distributed reduced solve (replaces CalculateGn,
// BundleAdjuster.cpp:748-833, across the GPUs of a node): the driver.  Device plumbing only —
// allocate, upload a table, launch, record, wait.  Ownership, the message plan, the per-panel steps and every table
// uploaded here: dist_plan.h; launch shapes: chol_launch.h; the factorisation kernels: k_chol.hip (chol_kernels.h);
// the design: DESIGN.md 6a.  Four streams per rank:
//   chain  (e->stream, chain communicator)  squares, their broadcast, the urgent block row and its messages;
//   panel  (e->stream2)  the other own rows of a panel, packing of their messages, the update of column block J+1;
//   side   (dist.stream4, side communicator)  those messages, point to point, and their unpacking;
//   bulk   (dist.stream3)  panel J applied to the own tiles right of column block J+1 (k_update128).
// The forward substitution rides along (the rhs row is a row of every square); the backward substitution walks the
// panels from the last: partial sums over the own tiles, one small all-reduce, then the square's own rows — the step
// is bitwise equal on all ranks.  Enabled when the caller installed the collectives hook (ba_hip_set_collectives) or
// the native communicator, more than one rank takes part, and the reduced system need not stay readable
// (keep_reduced_system).  BA_HIP_DIST_LAYOUT = tri | grid | col | row overrides the layout.
#include "chol_kernels.h"
#include <algorithm>
#include <vector>

namespace bae {

static const int NB = 64;        // tile size
static_assert(kTile == (uint32_t)NB && kDistTile == (uint32_t)NB, "chol_launch.h, dist_plan.h against the kernels");
static_assert(sizeof(DistPair) == sizeof(uint2) && sizeof(DistRect) == sizeof(uint4), "dist_plan.h tables as device vectors");

bool dist_solve_enabled(const Engine* e) {
  return e->coll && e->sharded() && !e->opt.keep_reduced_system && !chol_process_switches().no_dist_solve;
}

// a list of 64-row tiles (then, if the grid says so, the rhs row = row n_pad) x columns [c0, c0 + w) of A
// <->  dense row-major block in buf: messages carry no structurally zero tiles
__global__ void __launch_bounds__(256)
k_copy_panel_rows(double* __restrict__ A, uint32_t ld, const uint32_t* __restrict__ tiles, uint32_t ntiles,
                  uint32_t n_pad, uint32_t c0, uint32_t w, double* __restrict__ buf, int unpack) {
  const uint32_t r = blockIdx.x;
  const uint32_t arow = (r < ntiles * NB) ? tiles[r >> 6] * NB + (r & 63u) : n_pad;
  double* row = A + (size_t)arow * ld + c0;
  double* brow = buf + (size_t)r * w;
  for (uint32_t cc = threadIdx.x; cc < w; cc += 256) {
    if (unpack) row[cc] = brow[cc];
    else brow[cc] = row[cc];
  }
}

// a host table on the device (synchronous; at least one element is allocated)
template <typename T, typename U>
static int upload_table(Engine* e, DBuf<T>& d, const std::vector<U>& v) {
  static_assert(sizeof(T) == sizeof(U), "element sizes");
  BAE_HIP(d.alloc(std::max<size_t>(v.size(), 1)));
  if (!v.empty()) BAE_HIP(hipMemcpy(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// ---- the plan of the distributed solve for the current pattern / communicator, and its tables -------------
static int ensure_dist_plan(const CholSwitches& sw, Engine* e, uint32_t nblk, bool pat) {
  Engine::Dist& d = e->dist;
  const uint64_t want = dist_plan_key(e->nzL_version, sw.kout, pat, sw.dist_layout, sw.dense_scatter);
  if (d.key == want && d.plan.nblk == nblk && d.plan.map.n == (uint32_t)e->nranks && d.plan.map.rank == (uint32_t)e->rank)
    return 0;
  OwnMap map;
  std::string why;
  if (!build_own_map((uint32_t)e->nranks, sw.dist_layout, sw.kout, &map, &e->dist_layout_name, &why)) {
    e->err = "distributed solve: " + why;
    return -1;
  }
  map.rank = (uint32_t)e->rank;
  // one rank with the native communicator (comm_force): the rank sends its rows to itself — every pack /
  // transfer / unpack path runs on a one-GPU box
  d.plan = build_dist_plan(nblk, map, pat ? e->nzL_host.data() : nullptr, e->nranks == 1);
  d.tab = DistTables(d.plan);
  int rc = upload_table(e, d.tiles, d.plan.tiles);
  if (!rc) rc = upload_table(e, d.pairs, d.tab.own.pairs);
  if (!rc) rc = upload_table(e, d.square_rows, d.tab.square_rows);
  if (rc) return rc;
  d.key = want;
  return 0;
}

// Reduce-scatter of S onto the owners of its tile blocks.  Only the row tiles of a panel that hold a
// structurally nonzero tile of S on SOME shard travel (the union pattern of factor_tile_pattern, identical
// on every rank; S itself is half as dense as its factor): the other tiles are zero on every rank already.
static int dist_scatter_S_sparse(const CholSwitches& sw, Engine* e);
int dist_reduce_scatter_S(Engine* e) {
  const uint32_t ld = e->st.ld, nblk = ld / NB, N = (uint32_t)e->nranks, rank = (uint32_t)e->rank;
  const CholSwitches sw = chol_switches(nblk);
  // default: the sparse point-to-point exchange (below); BA_HIP_DENSE_SCATTER=1: one reduce-scatter of the union pattern
  if (!sw.dense_scatter && e->nranks > 1) return dist_scatter_S_sparse(sw, e);
  const bool pat = e->nzS_host.size() == (size_t)nblk * nblk;
  { const int prc = ensure_dist_plan(sw, e, nblk, pat && e->nzL_host.size() == (size_t)nblk * nblk); if (prc) return prc; }
  Engine::Dist& d = e->dist;
  const DistPlan& pl = d.plan;
  if (!d.tab.have_dense) {
    d.tab.dense = dist_dense_scatter_rows(pl, pat ? e->nzS_host.data() : nullptr);
    { const int urc = upload_table(e, d.dense_rows, d.tab.dense.rows); if (urc) return urc; }
    d.tab.have_dense = true;
  }
  const DistDenseRows& t = d.tab.dense;
  const size_t chunk = t.chunk;
  BAE_HIP(e->packed.alloc(chunk * N));
  // the padding behind the shorter chunks is summed too: keep it finite
  BAE_HIP(hipMemsetAsync(e->packed.p, 0, chunk * N * sizeof(double), e->stream));
  // the rows of (panel p, rank r) between A and their place in the chunk of r
  auto copy = [&](uint32_t p, uint32_t r, int unpack) {
    const size_t k = (size_t)p * N + r;
    const uint32_t ntl = t.off[k + 1] - t.off[k];
    if (ntl == 0) return;
    hipLaunchKernelGGL(k_copy_panel_rows, dim3(ntl * NB), dim3(256), 0, e->stream, e->A.p, ld,
                       (const uint32_t*)(d.dense_rows.p + t.off[k]), ntl, nblk * NB, pl.panels[p].c0 * NB,
                       (pl.panels[p].c1 - pl.panels[p].c0) * NB, e->packed.p + (size_t)r * chunk + t.chunk_off[k], unpack);
  };
  for (uint32_t p = 0; p < pl.nb; ++p)
    for (uint32_t r = 0; r < N; ++r) copy(p, r, 0);
  BAE_HIP(hipGetLastError());
  BAE_HIP(hipStreamSynchronize(e->stream));
  e->cstats.reduce_scatter_bytes += 8.0 * (double)chunk * N;
  if (e->coll(e->coll_ctx, 2, e->packed.p, chunk, 0) != 0) return e->fail_msg("reduce-scatter hook failed");
  for (uint32_t p = 0; p < pl.nb; ++p) copy(p, rank, 1);
  BAE_HIP(hipGetLastError());
  return 0;
}

// ---- sparse exchange of S: only the tiles a shard really has ------------------------------------------------------
// rects[b >> 6] = (row tile, first column in doubles, columns, offset of the 64 x columns block in buf);
// mode 0: buf <- A (pack), mode 1: A += buf (sum at the owner)
__global__ void __launch_bounds__(256)
k_copy_rects(double* __restrict__ A, uint32_t ld, const uint4* __restrict__ rects, double* __restrict__ buf, int mode) {
  const uint4 rc = rects[blockIdx.x >> 6];
  const uint32_t r = blockIdx.x & 63u;
  double* row = A + ((size_t)rc.x * NB + r) * ld + rc.y;
  double* brow = buf + (size_t)rc.w + (size_t)r * rc.z;
  for (uint32_t cc = threadIdx.x; cc < rc.z; cc += 256) {
    if (mode) row[cc] += brow[cc];
    else brow[cc] = row[cc];
  }
}

// Every rank holds a partial S over its landmark shard; the owner of a tile block needs the SUM.  Here a rank sends a
// (row tile x panel) rectangle to its owner only if its OWN pattern (Structure::tile_nz: the tiles its shard, its
// pose-pose residuals and the diagonal touch) has a tile in it (dist_sparse_rects); the owner adds what arrives in
// ascending rank order (deterministic).  With shards dealt along the trajectory a shard touches a band of S and
// sends a fraction of what the dense exchange does.  The local patterns are all-gathered once per plan (one u64
// all-reduce with every rank's bits in its own slot).
static int dist_scatter_S_sparse(const CholSwitches& sw, Engine* e) {
  const uint32_t ld = e->st.ld, nblk = ld / NB, N = (uint32_t)e->nranks, rank = (uint32_t)e->rank;
  { const int prc = ensure_dist_plan(sw, e, nblk, e->nzL_host.size() == (size_t)nblk * nblk); if (prc) return prc; }
  Engine::Dist& d = e->dist;
  if (e->st.tile_nz.size() != (size_t)nblk * nblk) return e->fail_msg("sparse exchange of S: no local tile pattern");
  if (!d.tab.have_sparse) {
    const size_t words = dist_pattern_words(nblk);
    std::vector<unsigned long long> all(words * N, 0ull);
    dist_pack_pattern(e->st.tile_nz.data(), nblk, all.data() + (size_t)rank * words);
    {
      DBuf<unsigned long long> dev;
      BAE_HIP(dev.alloc(all.size()));
      hipError_t err = hipMemcpy(dev.p, all.data(), all.size() * 8, hipMemcpyHostToDevice);
      int rc = 0;
      if (err != hipSuccess) rc = e->fail(err, "hipMemcpy");
      if (!rc && shard_allreduce(e, dev.p, all.size(), 1) != 0) rc = e->fail_msg("allreduce hook failed");
      if (!rc && (err = hipMemcpy(all.data(), dev.p, all.size() * 8, hipMemcpyDeviceToHost)) != hipSuccess) rc = e->fail(err, "hipMemcpy");
      if (rc) return rc;
    }
    d.tab.sparse = dist_sparse_rects(d.plan, rank, all.data(), words);
    if (!d.tab.sparse.refused.empty()) return e->fail_msg(d.tab.sparse.refused.c_str());
    int rc = upload_table(e, d.send_rects, d.tab.sparse.send);
    if (!rc) rc = upload_table(e, d.recv_rects, d.tab.sparse.recv);
    if (rc) return rc;
    d.tab.have_sparse = true;
  }
  const DistSparseRects& t = d.tab.sparse;
  const size_t stot = t.send_off[N], rtot = t.recv_off[N];
  // staging: the send half and the receive half of `packed`
  BAE_HIP(e->packed.alloc(std::max<size_t>(stot + rtot, 1)));
  double* sbuf = e->packed.p;
  double* rbuf = e->packed.p + stot;
  std::vector<DistXfer> xf;
  for (uint32_t peer = 0; peer < N; ++peer) {
    if (peer == rank) continue;
    const uint32_t ns = t.send_first[peer + 1] - t.send_first[peer];
    const size_t slen = t.send_off[peer + 1] - t.send_off[peer];
    if (ns) {
      hipLaunchKernelGGL(k_copy_rects, dim3(ns * 64), dim3(256), 0, e->stream, e->A.p, ld,
                         (const uint4*)(d.send_rects.p + t.send_first[peer]), sbuf, 0);
      xf.push_back({sbuf + t.send_off[peer], slen, (int)peer, true});
    }
    const size_t rlen = t.recv_off[peer + 1] - t.recv_off[peer];
    if (rlen) xf.push_back({rbuf + t.recv_off[peer], rlen, (int)peer, false});
  }
  BAE_HIP(hipGetLastError());
  e->cstats.reduce_scatter_bytes += 8.0 * (double)stot;
  {
    // (counted as the S exchange, not as chain traffic: undo dist_exchange's own bookkeeping)
    const ba_hip_comm_stats keep = e->cstats;
    const int xrc = dist_exchange(e, xf, false, e->stream);
    const double rs = e->cstats.reduce_scatter_bytes;
    e->cstats = keep;
    e->cstats.reduce_scatter_bytes = rs;
    if (xrc) return xrc;
  }
  for (uint32_t peer = 0; peer < N; ++peer) {   // ascending rank order: the sums are reproducible
    if (peer == rank) continue;
    const uint32_t nr = t.recv_first[peer + 1] - t.recv_first[peer];
    if (nr)
      hipLaunchKernelGGL(k_copy_rects, dim3(nr * 64), dim3(256), 0, e->stream, e->A.p, ld,
                         (const uint4*)(d.recv_rects.p + t.recv_first[peer]), rbuf, 1);
  }
  BAE_HIP(hipGetLastError());
  return 0;
}

// The tiles this rank's assembly has to write under the sparse exchange (dist_assembly_need).  Returns 1 if the
// restriction applies (distributed solve with the sparse exchange).
int dist_assembly_tiles(Engine* e, std::vector<uint8_t>* need) {
  const uint32_t nt = e->st.ld / NB;
  const CholSwitches sw = chol_switches(nt);
  if (!dist_solve_enabled(e) || e->nranks <= 1 || sw.dense_scatter) return 0;
  if (e->nzL_host.size() != (size_t)nt * nt || e->st.tile_nz.size() != (size_t)nt * nt) return 0;
  if (ensure_dist_plan(sw, e, nt, true)) return -1;
  *need = dist_assembly_need(e->dist.plan, (uint32_t)e->rank, e->st.tile_nz.data(), e->nzL_host.data());
  return 1;
}

// Backward substitution of the distributed solve, panel [c0, c1): partial sums over the row tiles this rank
// owns below the square,  part[g][col] = sum over its tiles t = g, g + NG, ... of  L[t-rows, col]^T x[t-rows].
__global__ void __launch_bounds__(256)
k_back_partial(const double* __restrict__ A, uint32_t ld, uint32_t nblk, const uint32_t* __restrict__ tiles,
               uint32_t ntiles, uint32_t c0, uint32_t w, const double* __restrict__ x,
               const uint8_t* __restrict__ nz, double* __restrict__ part) {
  __shared__ double xs[NB];
  const uint32_t col = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, ng = gridDim.y;
  double s = 0.0;
  for (uint32_t t = g; t < ntiles; t += ng) {
    const uint32_t i = tiles[t];
    __syncthreads();
    if (threadIdx.x < NB) xs[threadIdx.x] = x[(size_t)i * NB + threadIdx.x];
    __syncthreads();
    if (col < w && (!nz || nz[(size_t)i * nblk + c0 + (col >> 6)])) {
      const double* L = A + ((size_t)i * NB) * ld + (size_t)c0 * NB + col;
#pragma unroll 16
      for (int r = 0; r < NB; ++r) s += L[(size_t)r * ld] * xs[r];
    }
  }
  if (col < w) part[(size_t)g * w + col] = s;
}

// out[col] = sum over g (fixed order) of part[g][col]
__global__ void k_back_sum(const double* __restrict__ part, uint32_t ng, uint32_t w, double* __restrict__ out) {
  const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= w) return;
  double s = 0.0;
  for (uint32_t g = 0; g < ng; ++g) s += part[(size_t)g * w + col];
  out[col] = s;
}

// y[c0*64 + col] -= p[col]   (y = the rhs row of A)
__global__ void k_back_apply(double* __restrict__ yrow, const double* __restrict__ p, uint32_t w) {
  const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col < w) yrow[col] -= p[col];
}

int cholesky_solve_dist(Engine* e, double* dA, uint32_t ld, double* dx, int* status, const uint8_t* nz) {
  const uint32_t nblk = ld / NB, rank = (uint32_t)e->rank;
  const CholSwitches sw = chol_switches(nblk);
  const FactorWork fw(nblk);
  BAE_HIP(e->invdiag.alloc(fw.total));
  double* dsgn = e->invdiag.p + fw.dsgn;
  double* linvT = e->invdiag.p + fw.linvT;
  double* opbuf = e->invdiag.p + fw.opbuf;
  int* colneg = reinterpret_cast<int*>(e->invdiag.p + fw.colneg);
  const bool pat = nz && e->nzL_host.size() == (size_t)nblk * nblk;
  { const int prc = ensure_dist_plan(sw, e, nblk, pat); if (prc) return prc; }
  Engine::Dist& d = e->dist;
  const DistPlan& pl = d.plan;
  const DistOwnedPairs& op = d.tab.own;
  const OwnMap& own = pl.map;
  const uint32_t KOUT = own.G, npanels = pl.nb, n_pad = nblk * NB;
  const uint32_t* dtiles = d.tiles.p;
  // streams: chain, panel, bulk, side
  if (!d.stream3) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    BAE_HIP(hipStreamCreateWithPriority(&d.stream3, hipStreamNonBlocking, lo));
    BAE_HIP(hipStreamCreateWithPriority(&d.stream4, hipStreamNonBlocking, hi));
  }
  // (a native communicator without its duplicate — librccl lacks ncclCommSplit, or BA_HIP_ONE_COMM — carries the
  // side transfers too: they are then ordered into the chain stream, one communicator is never used on two streams)
  hipStream_t s0 = e->stream, s1 = e->stream2, s2 = d.stream3, s3 = (e->comm && !d.comm2) ? e->stream : d.stream4;
  // staging buffers: the square message; urgent / side messages of the busiest panel
  const size_t wmax = (size_t)KOUT * NB;
  BAE_HIP(d.msg.alloc(dist_square_doubles(KOUT)));
  BAE_HIP(d.usend.alloc(d.tab.caps.usend)); BAE_HIP(d.urecv.alloc(d.tab.caps.urecv));
  BAE_HIP(d.ssend.alloc(d.tab.caps.ssend)); BAE_HIP(d.srecv.alloc(d.tab.caps.srecv));
  const uint32_t NG = 32;
  BAE_HIP(d.back.alloc((size_t)(NG + 1) * wmax));
  while (d.ev.size() < (size_t)npanels * 5) {
    hipEvent_t a;
    BAE_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
    d.ev.push_back(a);
  }
  auto EV = [&](uint32_t J, int k) { return d.ev[(size_t)J * 5 + k]; };  // 0 urgent 1 packed 2 side 3 next 4 bulk
  e->cstats.factorisations++;
  { const int src = setup_status_block(e, dA, ld, s0); if (src) return src; }
  // everything queued on the chain stream so far (assembly, reduce-scatter unpack) precedes the other streams' work
  BAE_HIP(hipEventRecord(d.ev[1], s0));
  BAE_HIP(hipStreamWaitEvent(s1, d.ev[1], 0));
  BAE_HIP(hipStreamWaitEvent(s2, d.ev[1], 0));
  BAE_HIP(hipStreamWaitEvent(s3, d.ev[1], 0));
  if (rank == pl.panels[0].diag_owner)  // factor packet of tile 0
    launch_step_update(s0, dim3(1, 1), dA, ld, nblk, 0u, 0u, 0u, dsgn, opbuf, colneg, e->flags.p, nz, nullptr);
  // row list of a square: its tiles, then the rhs row — one small device array per plan (dist_square_rows)
  const DBuf<uint32_t>& sq_list = d.square_rows;
  int rc = 0;
  size_t sq_off = 0;
  for (uint32_t J = 0; J < npanels && !rc; ++J) {
    const DistPanel& pn = pl.panels[J];
    const uint32_t c0 = pn.c0, c1 = pn.c1, wt = c1 - c0, w = wt * NB;
    const uint32_t* sq = sq_list.p + sq_off;
    sq_off += wt + 1;
    const bool last = c1 >= nblk;
    // ---- chain stream: the square ----------------------------------------------------------------------
    double* msg = d.msg.p;
    const size_t n_cols = (size_t)(w + 1) * w;
    double* m_sgn = msg + n_cols;
    double* m_neg = m_sgn + w;
    double* m_op = m_neg + wt;
    const size_t msg_len = n_cols + w + wt + (size_t)wt * kPacketStride;
    if (rank == pn.diag_owner) {
      // (its updates by the earlier panels: bulk of steps <= J-2 and the chain-stream update of step J-1,
      // both ordered before this point by the waits of step J-1)
      launch_panel_chain(sw, s0, dA, ld, nblk, c0, c1, dsgn, opbuf, colneg, e->flags.p, nz, sq, wt + 1, true);
      hipLaunchKernelGGL(k_copy_panel_rows, dim3(w + 1), dim3(256), 0, s0, dA, ld, sq, wt, n_pad, c0 * NB, w, msg, 0);
      BAE_HIP(hipMemcpyAsync(m_sgn, dsgn + (size_t)c0 * NB, w * sizeof(double), hipMemcpyDeviceToDevice, s0));
      BAE_HIP(hipMemcpyAsync(m_neg, colneg + c0, wt * sizeof(int), hipMemcpyDeviceToDevice, s0));
      BAE_HIP(hipMemcpyAsync(m_op, opbuf + (size_t)c0 * kPacketStride, (size_t)wt * kPacketStride * sizeof(double),
                             hipMemcpyDeviceToDevice, s0));
    }
    BAE_HIP(hipGetLastError());
    if ((rc = dist_broadcast(e, msg, msg_len, (int)pn.diag_owner, s0))) break;
    if (rank != pn.diag_owner) {
      hipLaunchKernelGGL(k_copy_panel_rows, dim3(w + 1), dim3(256), 0, s0, dA, ld, sq, wt, n_pad, c0 * NB, w, msg, 1);
      BAE_HIP(hipMemcpyAsync(dsgn + (size_t)c0 * NB, m_sgn, w * sizeof(double), hipMemcpyDeviceToDevice, s0));
      BAE_HIP(hipMemcpyAsync(colneg + c0, m_neg, wt * sizeof(int), hipMemcpyDeviceToDevice, s0));
      BAE_HIP(hipMemcpyAsync(opbuf + (size_t)c0 * kPacketStride, m_op, (size_t)wt * kPacketStride * sizeof(double),
                             hipMemcpyDeviceToDevice, s0));
    }
    if (last) break;
    // ---- chain stream: the urgent block row (block J+1 of panel J) -------------------------------------
    // its tiles took the updates of the panels < J on the panel stream (step J-1: column block J)
    if (pn.own_u_count[rank]) {
      if (J > 0) BAE_HIP(hipStreamWaitEvent(s0, EV(J - 1, 3), 0));
      launch_panel_chain(sw, s0, dA, ld, nblk, c0, c1, dsgn, opbuf, colneg, e->flags.p, nz, dtiles + pn.own_u_first[rank],
                         pn.own_u_count[rank], false);
    }
    auto run_messages = [&](bool urgent, hipStream_t sp, hipStream_t sc, double* sendbuf, double* recvbuf,
                            hipEvent_t packed_ev) -> int {
      // pack on `sp` (the stream that computed the rows), transfer + unpack on `sc`
      std::vector<DistXfer> xf;
      struct Unp { const uint32_t* tl; uint32_t n; double* buf; };
      std::vector<Unp> unp;
      size_t so = 0, ro = 0;
      for (uint32_t mi : pn.msgs) {
        const DistMsg& m = pl.msgs[mi];
        if (m.urgent != urgent) continue;
        const size_t cnt = (size_t)m.count * NB * w;
        if (m.src == rank) {
          hipLaunchKernelGGL(k_copy_panel_rows, dim3(m.count * NB), dim3(256), 0, sp, dA, ld, dtiles + m.first, m.count,
                             n_pad, c0 * NB, w, sendbuf + so, 0);
          for (uint32_t q : m.dst) xf.push_back({sendbuf + so, cnt, (int)q, true});
          so += cnt;
        }
        if (std::find(m.dst.begin(), m.dst.end(), rank) != m.dst.end()) {
          xf.push_back({recvbuf + ro, cnt, (int)m.src, false});
          unp.push_back({dtiles + m.first, m.count, recvbuf + ro});
          ro += cnt;
        }
      }
      BAE_HIP(hipGetLastError());
      if (sp != sc) {
        BAE_HIP(hipEventRecord(packed_ev, sp));
        BAE_HIP(hipStreamWaitEvent(sc, packed_ev, 0));
      }
      const int xrc = dist_exchange(e, xf, !urgent, sc);
      if (xrc) return xrc;
      for (const Unp& u : unp)
        hipLaunchKernelGGL(k_copy_panel_rows, dim3(u.n * NB), dim3(256), 0, sc, dA, ld, u.tl, u.n, n_pad, c0 * NB, w,
                           u.buf, 1);
      BAE_HIP(hipGetLastError());
      return 0;
    };
    if ((rc = run_messages(true, s0, s0, d.usend.p, d.urecv.p, nullptr))) break;
    BAE_HIP(hipEventRecord(EV(J, 0), s0));
    // ---- chain stream: panel J applied to the next square (and its rhs segment) + its first diagonal tile
    const uint32_t n1 = std::min(c1 + KOUT, nblk);  // end of column block J+1
    if (rank == pl.panels[J + 1].diag_owner) {
      if (J > 0) BAE_HIP(hipStreamWaitEvent(s0, EV(J - 1, 4), 0));  // the bulk updates of its tiles by the panels < J
      launch_step_update(s0, dim3(n1 - c1 + 1, n1 - c1), dA, ld, nblk, c1, c0, c1, dsgn, opbuf, colneg, e->flags.p, nz,
                         sq_list.p + sq_off);
    }
    // ---- panel stream: the other own rows of panel J, their messages -----------------------------------
    BAE_HIP(hipStreamWaitEvent(s1, EV(J, 0), 0));
    if (J > 0) BAE_HIP(hipStreamWaitEvent(s1, EV(J - 1, 2), 0));  // the side staging buffers are free again
    if (pn.own_r_count[rank])
      launch_panel_chain(sw, s1, dA, ld, nblk, c0, c1, dsgn, opbuf, colneg, e->flags.p, nz, dtiles + pn.own_r_first[rank],
                         pn.own_r_count[rank], false);
    if ((rc = run_messages(false, s1, s3, d.ssend.p, d.srecv.p, EV(J, 1)))) break;
    BAE_HIP(hipEventRecord(EV(J, 2), s3));
    // ---- panel stream: panel J applied to the own tiles of column block J+1 below its square ------------
    if (pn.next_needs_side[rank] || own.n <= 1) BAE_HIP(hipStreamWaitEvent(s1, EV(J, 2), 0));  // rows received on the side stream
    if (J > 0) BAE_HIP(hipStreamWaitEvent(s1, EV(J - 1, 4), 0));
    if (n1 < nblk) {
      const uint32_t ncols = n1 - c1;
      OwnMap o1 = own;
      o1.skip_rhs = 1;  // the rhs segment of column block J+1 went with the square's update on the chain stream
      const Rect128Shape r = rect128_shape(kRectDist, nblk, c1, ncols, own.G, sw);
      if (r.use128) {
        launch_rect128(sw, r, s1, dA, ld, nblk, c1, ncols, c0, c1, dsgn, colneg, nz, o1);
      } else {
        // 64-tiles: exactly the row tiles this rank owns below the square of panel J+1 (its two row lists are
        // adjacent) — a structurally zero tile of L takes no update, so the lists are complete
        const DistPanel& pq = pl.panels[J + 1];
        const uint32_t cnt = pq.own_u_count[rank] + pq.own_r_count[rank];
        if (cnt)
          launch_step_update(s1, dim3(cnt, ncols), dA, ld, nblk, c1, c0, c1, dsgn, opbuf, colneg, e->flags.p, nz,
                             dtiles + pq.own_u_first[rank]);
      }
    }
    BAE_HIP(hipEventRecord(EV(J, 3), s1));
    // ---- bulk stream: panel J applied to the own tiles right of column block J+1 -----------------------
    if (n1 < nblk) {
      BAE_HIP(hipStreamWaitEvent(s2, EV(J, 2), 0));
      BAE_HIP(hipStreamWaitEvent(s2, EV(J, 0), 0));
      launch_bulk_update(sw, e, s2, dA, ld, nblk, n1, c0, c1, dsgn, colneg, nz, true, own, d.pairs.p + op.pair_first[J],
                         (uint32_t)op.pairs.size() - op.pair_first[J]);
      if (e->profiling)   // tile products formed by THIS rank
        e->kstats.syrk_flops += bulk_update_tile_products(own, rank, nblk, n1, c0, c1, pat ? e->nzL_host.data() : nullptr) *
                                2.0 * NB * NB * NB;
    }
    BAE_HIP(hipEventRecord(EV(J, 4), s2));
  }
  if (rc) return rc;
  BAE_HIP(hipGetLastError());
  // every stream has drained into the chain stream's view before the backward substitution
  BAE_HIP(hipStreamSynchronize(s1));
  BAE_HIP(hipStreamSynchronize(s2));
  BAE_HIP(hipStreamSynchronize(s3));
  launch_linvT(s0, nblk, opbuf, dsgn, linvT);
  // ---- backward substitution, panels from the last -------------------------------------------------------
  double* yrow = dA + (size_t)n_pad * ld;
  double* part = d.back.p;
  double* psum = part + (size_t)NG * wmax;
  for (uint32_t J = npanels; J-- > 0 && !rc;) {
    const DistPanel& pn = pl.panels[J];
    const uint32_t c0 = pn.c0, c1 = pn.c1, w = (c1 - c0) * NB;
    if (c1 < nblk) {
      const uint32_t nt = pn.own_u_count[rank] + pn.own_r_count[rank];  // (the two lists are adjacent)
      const uint32_t ng = std::min(NG, std::max(nt, 1u));
      if (nt) {
        hipLaunchKernelGGL(k_back_partial, dim3((w + 255) / 256, ng), dim3(256), 0, s0, (const double*)dA, ld, nblk,
                           dtiles + pn.own_u_first[rank], nt, c0, w, (const double*)dx, nz, part);
        hipLaunchKernelGGL(k_back_sum, dim3((w + 255) / 256), dim3(256), 0, s0, (const double*)part, ng, w, psum);
      } else {
        BAE_HIP(hipMemsetAsync(psum, 0, (size_t)w * sizeof(double), s0));
      }
      BAE_HIP(hipGetLastError());
      if ((rc = dist_allreduce_stream(e, psum, w, s0))) break;
      hipLaunchKernelGGL(k_back_apply, dim3((w + 255) / 256), dim3(256), 0, s0, yrow + (size_t)c0 * NB, (const double*)psum, w);
    }
    launch_backward(s0, dA, ld, nblk, (const double*)linvT, dx, nz, c0, c1);
  }
  if (rc) return rc;
  BAE_HIP(hipGetLastError());
  // the pivot status of every diagonal owner
  int st = 0;
  BAE_HIP(hipMemcpyAsync(&st, e->flags.p, sizeof(int), hipMemcpyDeviceToHost, s0));
  BAE_HIP(hipStreamSynchronize(s0));
  double sd = (double)st;
  BAE_HIP(hipMemcpy(e->scalars_out.p, &sd, sizeof(double), hipMemcpyHostToDevice));
  if (shard_allreduce(e, e->scalars_out.p, 1, 0) != 0) return e->fail_msg("allreduce hook failed");
  BAE_HIP(hipMemcpy(&sd, e->scalars_out.p, sizeof(double), hipMemcpyDeviceToHost));
  *status = sd > 0.5 ? 1 : 0;
  return 0;
}

}  // namespace bae
