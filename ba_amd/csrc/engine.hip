// Host side of the gfx950 engine: C-ABI entry points of include/ba_hip.h, the
// per-Solve structure build (observation CSR, incidences, gather lists) and the phase
// drivers that enqueue the kernels of k_proj.hip / k_reduce.hip / k_chol.hip.
#include "entry.h"
#include <chrono>
#include <functional>
#include <memory>
#include <thread>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "dmath.h"
#include "factorsolve.h"
#include "dpose.h"

namespace bae {

int Engine::fail(hipError_t e, const char* what) {
  err = std::string(what) + ": " + hipGetErrorString(e);
  return -(int)(e == hipSuccess ? 1 : e);
}
void Engine::prof_collect() {
  auto drain = [](std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, double& ms, uint32_t& n) {
    for (auto& p : v) {
      (void)hipEventSynchronize(p.second);
      float t = 0;
      (void)hipEventElapsedTime(&t, p.first, p.second);
      ms += t; n += 1;
      (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second);
    }
    v.clear();
  };
  drain(ev_syrk, kstats.syrk_ms, kstats.syrk_launches);
  drain(ev_gather, kstats.gather_ms, kstats.gather_launches);
  drain(ev_landmarks, kstats.landmarks_ms, kstats.landmarks_launches);
  drain(ev_imu, kstats.imu_ms, kstats.imu_launches);
  drain(ev_pose, kstats.pose_blocks_ms, kstats.pose_blocks_launches);
}
int Engine::fail_msg(const char* what) {
  err = what;
  return -1;
}
Engine::~Engine() {
  for (hipStream_t s : {stream, stream2, dist.stream3, dist.stream4})
    if (s) (void)hipStreamSynchronize(s);
  for (auto* v : {&ev_panel, &ev_bulk, &dist.ev, &timer_events})
    for (hipEvent_t ev : *v) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : {ev_imu_start, ev_imu_done, ev_fork, ev_join})
    if (ev) (void)hipEventDestroy(ev);
  for (auto* v : {&ev_syrk, &ev_gather, &ev_landmarks, &ev_imu, &ev_pose})   // profiling pairs nobody collected
    for (auto& pr : *v) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (hipStream_t s : {stream2, dist.stream3, dist.stream4})
    if (s) (void)hipStreamDestroy(s);
  if (own_stream && stream) (void)hipStreamDestroy(stream);   // a caller's stream is only synchronised
}

static_assert(sizeof(U2) == sizeof(uint2) && sizeof(U3) == 3 * sizeof(uint32_t) && sizeof(U4) == sizeof(uint4),
              "list records are plain words");

// S: T itself, or the host record of structure.h with its layout (U4 for uint4)
template <typename T, typename S>
static int upload(Engine* e, DBuf<T>& buf, const std::vector<S>& v, size_t min_count = 0) {
  static_assert(sizeof(S) == sizeof(T), "host record and device element differ in size");
  const size_t n = std::max(v.size(), min_count);
  BAE_HIP(buf.alloc(std::max<size_t>(n, 1)));
  if (!v.empty()) {
    // the source is pageable host memory that the caller may free right after this returns (most
    // call sites pass short-lived vectors): the copy must have read it by then, so drain the stream
    BAE_HIP(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, e->stream));
    BAE_HIP(hipStreamSynchronize(e->stream));
  }
  return 0;
}

// Phase timer on the engine's stream.  The two events come from a pool the engine keeps (creating and
// destroying a pair per phase call cost a small window ~10 us each time).
struct EventTimer {
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t s;
  Engine* eng;
  explicit EventTimer(Engine* e) : s(e->stream), eng(e) {
    a = take();
    b = take();
    (void)hipEventRecord(a, s);
  }
  ~EventTimer() { give(); }  // (an error path that never read the timer)
  // mark(): the end point in stream order; read_ms(): wait for it and read — apart, so that a phase call
  // can mark several intervals and pay for ONE synchronisation at its end
  void mark() { (void)hipEventRecord(b, s); marked = true; }
  double stop_ms() { mark(); return read_ms(); }
  bool marked = false;
  double read_ms() {
    if (!a) return 0.0;
    if (!marked) mark();
    (void)hipEventSynchronize(b);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    give();
    return ms;
  }
 private:
  hipEvent_t take() {
    if (!eng->timer_events.empty()) { hipEvent_t ev = eng->timer_events.back(); eng->timer_events.pop_back(); return ev; }
    hipEvent_t ev = nullptr;
    (void)hipEventCreate(&ev);
    return ev;
  }
  void give() {
    if (a) eng->timer_events.push_back(a);
    if (b) eng->timer_events.push_back(b);
    a = b = nullptr;
  }
};

// gravity | measurement noise diag (gyro^2 x3, accel^2 x3) | bias random walk.  Not part of the
// structure: refreshed by every ba_hip_begin_solve, so SetGravity / SetImuCalibration / new option
// sigmas between two Solve() calls need no ba_hip_finalize.
static int upload_imu_consts(Engine* e) {
  const Problem& pb = e->prob;
  std::vector<double> c(15);
  for (int i = 0; i < 3; ++i) {
    c[i] = pb.gravity[i];
    c[3 + i] = e->opt.gyro_sigma * e->opt.gyro_sigma;
    c[6 + i] = e->opt.accel_sigma * e->opt.accel_sigma;
    c[9 + i] = e->opt.gyro_bias_sigma * e->opt.gyro_bias_sigma;
    c[12 + i] = e->opt.accel_bias_sigma * e->opt.accel_bias_sigma;
  }
  if (pb.imu_noise.size() == 12)  // ImuCalibrationT::r / r_b given explicitly (SetImuCalibration)
    for (int i = 0; i < 12; ++i) c[3 + i] = pb.imu_noise[i];
  return upload(e, e->imu_consts, c);
}

bool ordering_wants_graph(const Engine* e) { return e->order_mode == kOrderAuto; }

int order_poses(Engine* e, std::vector<uint64_t>* proj_edges, double device_ms) {
  const auto t0 = std::chrono::steady_clock::now();
  const Problem& pb = e->prob;
  std::vector<int32_t> nat;
  const uint32_t Pact = natural_pose_opt(pb, nat);
  ba_hip_ordering_stats& os = e->order_stats;
  os.mode = e->order_mode;
  os.device_ms = device_ms;
  if (e->order_mode == kOrderUser) {
    const std::vector<uint32_t>& u = e->order_user;
    if (u.size() != Pact) return e->fail_msg("ba_hip_set_pose_permutation: size differs from the active pose count");
    std::vector<uint8_t> seen(Pact, 0);
    for (uint32_t v : u) {
      if (v >= Pact || seen[v]) return e->fail_msg("ba_hip_set_pose_permutation: not a permutation of the active poses");
      seen[v] = 1;
    }
    e->opt_of_natural = u;
  } else {
    const int D = e->pose_dim;
    const uint32_t G = pose_group_size(D), ng = (Pact + G - 1) / G;
    // the projection part's group pairs, then those of the binary and inertial residuals and the dense priors
    std::vector<uint64_t> edges(proj_edges ? *proj_edges : std::vector<uint64_t>());
    const DensePriors& pr = e->dpri;
    coupling_group_edges(pb, pr.count(), pr.ptr.data(), pr.pose.data(), nat, G, edges);
    group_graph_csr(ng, std::move(edges), e->group_ptr, e->group_adj);
    OrderingResult r;
    choose_pose_ordering(Pact, D, (uint32_t)e->calib_dim, e->group_ptr, e->group_adj, e->opt_of_natural, &r);
    os.candidate = r.candidate;
    os.group_size = r.G;
    os.num_groups = ng;
    os.tile_products_natural = r.products[0];
    os.tile_products_chosen = r.products[r.candidate];
  }
  os.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

// ---- ba_hip_finalize: the steps of build_structure ---------------------------------------------------
// a buffer of at least one element, cleared in stream order
template <typename T>
static hipError_t alloc_zeroed(Engine* e, DBuf<T>& buf, size_t count) {
  const hipError_t err = buf.alloc(std::max<size_t>(count, 1));
  return err != hipSuccess ? err : hipMemsetAsync(buf.p, 0, buf.bytes(), e->stream);
}

#define UP(buf, vec) if ((rc = upload(e, e->buf, vec))) return rc

// the lists of build_lists (the device builder leaves its own on the device); frees the big host copies
static int upload_host_lists(Engine* e) {
  const Problem& pb = e->prob;
  Structure& st = e->st;
  int rc;
  UP(pose_opt, st.pose_opt); UP(lm_opt, st.lm_opt);
  UP(lm_ref_pose, pb.lm_ref_pose); UP(lm_ref_cam, pb.lm_ref_cam);
  UP(lm_ptr, st.lm_ptr); UP(obs_z, st.obs_z); UP(obs_pose, st.obs_pose); UP(obs_cam, st.obs_cam);
  UP(obs_lm, st.obs_lm); UP(obs_rid, st.obs_rid); UP(obs_w0, st.obs_w0);
  UP(tile_ptr, st.tile_ptr); UP(pose_ptr, st.pose_ptr); UP(pose_mid, st.pose_mid);
  BAE_HIP(e->pair_ent.alloc(std::max<size_t>(st.n_pair_entries, 1)));
  if (st.n_pair_entries)
    BAE_HIP(hipMemcpyAsync(e->pair_ent.p, st.pair_ent.get(), st.n_pair_entries * sizeof(uint2), hipMemcpyHostToDevice, e->stream));
  BAE_HIP(e->wave_rng.alloc(std::max<size_t>(st.n_chunks, 1)));
  if (st.n_chunks)
    BAE_HIP(hipMemcpyAsync(e->wave_rng.p, st.wave_rng.data(), (size_t)st.n_chunks * sizeof(uint2), hipMemcpyHostToDevice, e->stream));
  BAE_HIP(e->tile_ref.alloc(std::max<size_t>(st.n_tile_refs, 1)));
  if (st.n_tile_refs)
    BAE_HIP(hipMemcpyAsync(e->tile_ref.p, st.tile_ref.data(), st.n_tile_refs * sizeof(uint2), hipMemcpyHostToDevice, e->stream));
  BAE_HIP(e->pose_ent.alloc(std::max<size_t>(3 * st.n_pose_entries, 1)));
  if (st.n_pose_entries)
    BAE_HIP(hipMemcpyAsync(e->pose_ent.p, st.pose_ent.data(), st.n_pose_entries * sizeof(U3), hipMemcpyHostToDevice, e->stream));
  BAE_HIP(hipStreamSynchronize(e->stream));
  // the big host lists are only needed on the device from here on
  st.pair_ent.reset();
  std::vector<U2>().swap(st.tile_ref);
  std::vector<U3>().swap(st.pose_ent);
  std::vector<double>().swap(st.obs_z);
  // conditioning residuals (BundleAdjuster.h:503-510): flags in sorted order
  std::vector<uint8_t> is_cond(st.O, 0), cond_sorted(std::max<uint32_t>(st.O, 1), 0);
  for (uint32_t id : pb.proj_cond) if (id < st.O) is_cond[id] = 1;
  for (uint32_t s = 0; s < st.O; ++s) cond_sorted[s] = is_cond[st.obs_rid[s]];
  UP(obs_cond, cond_sorted);
  return 0;
}

// the unary / binary / inertial residuals, their scatter lists and per-slot buffers, the cameras
static int upload_pose_pose(Engine* e, const PosePoseLists& pp) {
  const Problem& pb = e->prob;
  int rc;
  UP(pose_active, pb.pose_active);
  UP(un_pose, pb.un_pose); UP(un_t, pb.un_t); UP(un_cov_inv, pb.un_cov_inv); UP(un_rot, pb.un_rot);
  UP(bin_p1, pb.bin_p1); UP(bin_p2, pb.bin_p2); UP(bin_t, pb.bin_t); UP(bin_cov_inv, pb.bin_cov_inv);
  UP(bin_cov_inv_sqrt, pb.bin_cov_inv_sqrt); UP(bin_w, pb.bin_w); UP(bin_rot, pb.bin_rot);
  UP(imu_p1, pb.imu_p1); UP(imu_p2, pb.imu_p2); UP(imu_ptr, pb.imu_ptr); UP(imu_meas, pb.imu_meas);
  UP(pp_ptr, pp.pp_ptr); UP(pp_ent, pp.pp_ent); UP(pp_res_p1, pp.res_p1); UP(pp_res_p2, pp.res_p2);
  const std::vector<double> ones(std::max<uint32_t>(pb.num_unary, 1), 1.0);
  UP(un_scale, ones);
  if ((rc = upload_imu_consts(e))) return rc;
  const size_t nr1 = std::max<size_t>(pp.res_p1.size(), 1);
  BAE_HIP(e->pp_h.alloc(nr1 * 3 * 225)); BAE_HIP(e->pp_g.alloc(nr1 * 30));
  BAE_HIP(e->pp_dz.alloc(nr1 * 2 * 225)); BAE_HIP(e->pp_info.alloc(nr1 * 225));
  BAE_HIP(e->pp_err.alloc(nr1));
  BAE_HIP(e->pp_err_lin.alloc(nr1));
  BAE_HIP(alloc_zeroed(e, e->imu_cov_inv, std::max<size_t>(pb.num_imu, 1) * 225));
  e->tvs_eval = pb.cam_tvs;
  e->tvs_eval_prev = pb.cam_tvs;
  return upload_cameras(e, false);
}
#undef UP

// the double-buffered state, the transforms derived from it, masks and outlier counts
static int alloc_state(Engine* e) {
  const Problem& pb = e->prob;
  const Structure& st = e->st;
  int rc;
  e->cur = 0;
  e->held.structure_rebuilt();   // (nothing since the new tile pattern has read the old one's flag)
  for (int b = 0; b < 2; ++b) {
    BAE_HIP(e->pose_state[b].alloc(std::max<size_t>((size_t)st.P * kPoseState, 1)));
    BAE_HIP(e->lm_x[b].alloc(std::max<size_t>((size_t)st.L * 4, 1)));
    BAE_HIP(e->lm_reliable[b].alloc(std::max<size_t>(st.L, 1)));
  }
  if (st.P) BAE_HIP(hipMemcpyAsync(e->pose_state[0].p, pb.pose_state.data(),
                                   (size_t)st.P * kPoseState * sizeof(double), hipMemcpyHostToDevice, e->stream));
  if ((rc = upload(e, e->lm_xw, pb.lm_xw))) return rc;
  if (st.L) {
    BAE_HIP(hipMemcpyAsync(e->lm_x[0].p, pb.lm_xw.data(), (size_t)st.L * 4 * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    BAE_HIP(hipMemsetAsync(e->lm_reliable[0].p, 1, st.L, e->stream));
  }
  const size_t PC = std::max<size_t>((size_t)st.P * std::max(st.C, 1u), 1);
  BAE_HIP(e->tsw.alloc(PC * kRt)); BAE_HIP(e->tws.alloc(PC * kRt));
  BAE_HIP(e->twp.alloc(std::max<size_t>((size_t)st.P * kRt, 1)));
  BAE_HIP(alloc_zeroed(e, e->pose_mask, (size_t)st.P + st.Pact));
  BAE_HIP(e->pose_mask_lin.alloc(std::max<size_t>((size_t)st.P + st.Pact, 1)));
  e->lin_mask_version = e->mask_version;   // no linearisation yet: nothing reads the copy
  BAE_HIP(alloc_zeroed(e, e->lm_outliers, st.L));
  return 0;
}

// what an iteration writes: residuals and factor rows, the reduced system, steps, reduction scratch
static int alloc_iteration_buffers(Engine* e, bool host_build) {
  const Problem& pb = e->prob;
  const Structure& st = e->st;
  int rc;
  const size_t O1 = std::max<size_t>(st.O, 1), L1 = std::max<size_t>(st.L, 1);
  const int LM1 = std::max(e->lm_dim, 1);
  BAE_HIP(e->obs_e.alloc(O1)); BAE_HIP(e->obs_w.alloc(O1));
  BAE_HIP(e->obs_jl.alloc(O1 * 2 * LM1));
  if (st.O && host_build) BAE_HIP(hipMemcpyAsync(e->obs_w.p, st.obs_w0.data(), (size_t)st.O * sizeof(double),
                                                 hipMemcpyHostToDevice, e->stream));
  BAE_HIP(alloc_zeroed(e, e->frow, (size_t)st.n_rows * kRow));
  BAE_HIP(alloc_zeroed(e, e->scal, std::max<size_t>(st.n_scalars, 2 * O1 + L1 * LM1 + 1)));  // last: the zero scalar
  if (st.K && !e->calib_tvs) {
    // parallel_algos.h:115-118 assigns dTransfer_dparams (2 x NumParams) to a 2 x CalibSize block
    const int nparams = (!pb.cam_model.empty() && pb.cam_model[0] == 1) ? 5 : 4;
    if ((int)st.K != nparams)
      return e->fail_msg("CalibSize must equal the parameter count of camera 0 (LinearCamera 4, FovCamera 5)");
    if (pb.lm_zref.size() != 2 * (size_t)st.L)
      return e->fail_msg("intrinsics calibration needs the reference pixel of every landmark (ba_hip_set_landmark_ref_pixels)");
    if ((rc = upload(e, e->lm_zref, pb.lm_zref))) return rc;
  }
  e->cam_params_prev = pb.cam_params;
  e->cam_w_prev = pb.cam_w;
  if (st.K) {
    BAE_HIP(alloc_zeroed(e, e->crow, std::max<size_t>(st.n_scalars, 1) * kRow));
    BAE_HIP(e->border_blocks.alloc(std::max<size_t>((size_t)st.Pact * 36, 1)));
  }
  BAE_HIP(alloc_zeroed(e, e->lm_vinv, L1 * LM1 * LM1));
  BAE_HIP(alloc_zeroed(e, e->lm_bl, L1 * LM1));
  BAE_HIP(e->A.alloc((size_t)(st.ld + 1) * st.ld));
  BAE_HIP(e->rhs_p.alloc(st.ld)); BAE_HIP(e->rhs_sc.alloc(st.ld));
  BAE_HIP(alloc_zeroed(e, e->gn_p, st.ld));
  BAE_HIP(alloc_zeroed(e, e->step_p, st.ld));
  const size_t nl = (size_t)st.Lact * LM1;
  BAE_HIP(alloc_zeroed(e, e->gn_l, nl));
  BAE_HIP(alloc_zeroed(e, e->step_l, nl));
  // reduction scratch: block partials of the element-wise kernels (up to 4 components) and one
  // partial per linearisation wave
  const size_t nparts = std::max<size_t>({(O1 + 255) / 256, (L1 + 255) / 256, (size_t)(st.ld + 255) / 256, 1});
  BAE_HIP(e->partials.alloc(std::max<size_t>(4 * nparts, st.n_chunks)));
  BAE_HIP(e->scalars_out.alloc(128));  // [0,64) results / staging, [64,128) first-level partial sums
  BAE_HIP(e->hist.alloc(2048 + 8));
  BAE_HIP(e->flags.alloc(16));
  return 0;
}

// Build everything that depends only on the problem graph (not on the state): the lists of
// structure.h (on the device, or on host threads), the pose-pose scatter lists, the tile pattern; then
// upload and size the buffers.
static int build_structure(Engine* e) {
  Problem& pb = e->prob;
  Structure& st = e->st;
  // BA_HIP_DEBUG_SETUP: wall-clock of the stages of the structure build on stderr
  static const bool dbg_setup = getenv("BA_HIP_DEBUG_SETUP") != nullptr;
  auto t_stage = std::chrono::steady_clock::now();
  auto stage = [&](const char* name) {
    if (!dbg_setup) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[setup] %-28s %.3f s\n", name, std::chrono::duration<double>(now - t_stage).count());
    t_stage = now;
  };
  const int LM = e->lm_dim;
  // the static lists: on the device (structure_dev.hip) unless BA_HIP_HOST_STRUCTURE / debug key 5
  // asks for the host builder (structure.h: the executable specification, same lists)
  static const bool env_host = getenv("BA_HIP_HOST_STRUCTURE") != nullptr;
  const bool host_build = env_host || e->dbg_host_structure;
  if (host_build) {
    std::string err;
    if (e->order_mode != kOrderNatural) {
      std::vector<uint64_t> edges;
      if (ordering_wants_graph(e)) {
        std::vector<int32_t> nat;
        natural_pose_opt(pb, nat);
        host_group_edges(pb, LM, nat, pose_group_size(e->pose_dim), edges);
      }
      const int orc = order_poses(e, &edges, 0.0);
      if (orc) return orc;
      stage("pose ordering");
    }
    if (!build_lists(pb, LM, e->pose_dim, st, err, stage, e->calib_dim, &e->opt_of_natural)) {
      e->err = err;
      return -1;
    }
  } else {
    const int brc = build_lists_device(e, stage);
    if (brc) return brc;
  }
  PosePoseLists pp;
  {
    std::string err;
    if (!build_pose_pose_lists(pb, st, pp, err)) return e->fail_msg(err.c_str());
  }
  stage("pose-pose lists");
  int rc;
  if ((rc = priors_upload(e))) return rc;
  // 64x64-tile pattern of S (for the tile-sparse factorisation): the list builder marked the tiles of the
  // projection part and the diagonal; add the pose-pose residuals, the dense priors and the calibration border
  mark_pose_pose_tiles(pb, e->dpri.count(), e->dpri.ptr.data(), e->dpri.pose.data(), e->pose_dim, st);
  stage("tile pattern");
  if (host_build && (rc = upload_host_lists(e))) return rc;
  if ((rc = upload_pose_pose(e, pp))) return rc;
  if ((rc = alloc_state(e))) return rc;
  if ((rc = alloc_iteration_buffers(e, host_build))) return rc;
  BAE_HIP(hipStreamSynchronize(e->stream));
  stage("upload / device buffers");
  return 0;
}

// Launch order of the tile assembly (k_assemble_tiles).  Only tiles of the factor's pattern are
// written every iteration: the others are zero since the one-off clear of the square and nobody ever
// writes them (the factorisation skips structurally zero tiles).  Order: blocks b, b + 8, .. share
// an XCD; XCD x gets the tile columns I = x, x + 8, .. and walks each from the diagonal down, so the
// tiles in flight on one XCD gather the same pose group's rows out of its L2.
int build_tile_order(Engine* e) {
  const Structure& st = e->st;
  if (!e->held.nzL_valid) {
    int rc = factor_tile_pattern(e);
    if (rc) return rc;
  }
  const uint32_t nt = st.ld / 64;
  // distributed solve with the sparse exchange of S: only the tiles this rank owns or sends (dist_solve.hip)
  std::vector<uint8_t> need;
  const int restricted = e->dbg_all_tiles ? 0 : dist_assembly_tiles(e, &need);
  if (restricted < 0) return restricted;
  const uint64_t plan_key = restricted ? e->dist.key : ~0ull;
  if (e->tile_order_version == e->nzL_version && e->tile_order.p && e->tile_order_plan == plan_key) return 0;
  const bool pat = !e->dbg_all_tiles && e->nzL_host.size() == (size_t)nt * nt;
  const std::vector<uint8_t>& which = restricted ? need : e->nzL_host;
  std::vector<uint32_t> order;
  size_t longest = 0;
  if (e->dbg_tile_order == 1) {
    std::vector<std::vector<uint32_t>> queue(8);
    for (uint32_t I = 0; I < nt; ++I)
      for (uint32_t J = I; J < nt; ++J)
        if (!pat || which[(size_t)J * nt + I]) queue[I % 8].push_back((uint32_t)((uint64_t)J * (J + 1) / 2 + I));
    for (auto& q : queue) longest = std::max(longest, q.size());
    order.assign(std::max<size_t>(8 * longest, 1), 0xffffffffu);
    for (uint32_t x = 0; x < 8; ++x)
      for (size_t k = 0; k < queue[x].size(); ++k) order[8 * k + x] = queue[x][k];
  } else {
    // row-major over the lower tiles: a tile row mixes gather-heavy tiles near the diagonal band with
    // fill-only tiles, so latency-bound and bandwidth-bound workgroups overlap on every CU
    for (uint32_t J = 0; J < nt; ++J)
      for (uint32_t I = 0; I <= J; ++I)
        if (!pat || which[(size_t)J * nt + I]) order.push_back((uint32_t)((uint64_t)J * (J + 1) / 2 + I));
    longest = (order.size() + 7) / 8;
    order.resize(std::max<size_t>(8 * longest, 1), 0xffffffffu);
  }
  e->n_tile_order = (uint32_t)(8 * longest);
  int rc = upload(e, e->tile_order, order);
  if (rc) return rc;
  if ((rc = build_tile_desc(e))) return rc;
  e->tile_order_version = e->nzL_version;
  e->tile_order_plan = plan_key;
  return 0;
}

// cameras: params(4) | T_vs Rt(12) | T_sv Rt(12) | T_vs as t,q (7) | w | model (kCamRec doubles); `cam` from
// the rig (prob.cam_tvs), cam_eval (calibration only) from tvs_eval
int upload_cameras(Engine* e, bool eval_only) {
  const Problem& pb = e->prob;
  const uint32_t C = pb.num_cams;
  auto table = [&](const std::vector<double>& tvs) {
    std::vector<double> cam((size_t)C * kCamRec, 0.0);
    for (uint32_t c = 0; c < C; ++c) {
      double* o = &cam[(size_t)c * kCamRec];
      const double* t = &tvs[(size_t)c * 7];
      for (int i = 0; i < 4; ++i) o[i] = pb.cam_params[(size_t)c * 4 + i];
      bad::Rt vs;
      vs.R = bad::quat_to_rot(t[3], t[4], t[5], t[6]);
      vs.t = bad::v3(t[0], t[1], t[2]);
      const bad::Rt sv = bad::inverse(vs);
      for (int i = 0; i < 9; ++i) { o[4 + i] = vs.R.m[i]; o[16 + i] = sv.R.m[i]; }
      o[13] = vs.t.x; o[14] = vs.t.y; o[15] = vs.t.z;
      o[25] = sv.t.x; o[26] = sv.t.y; o[27] = sv.t.z;
      for (int i = 0; i < 7; ++i) o[28 + i] = t[i];
      const bool fov = c < pb.cam_model.size() && pb.cam_model[c] == 1;
      o[35] = fov ? pb.cam_w[c] : 0.0;
      o[36] = fov ? 1.0 : 0.0;
    }
    return cam;
  };
  e->has_fov = false;
  for (uint32_t c = 0; c < C && c < pb.cam_model.size(); ++c) e->has_fov |= pb.cam_model[c] == 1;
  int rc;
  if (!eval_only && (rc = upload(e, e->cam, table(pb.cam_tvs)))) return rc;
  if (e->calib_dim && (rc = upload(e, e->cam_eval, table(e->tvs_eval)))) return rc;
  return 0;
}

static int set_masks_device(Engine* e, const std::vector<uint16_t>& by_id) {
  const Structure& st = e->st;
  // the factor in A stays readable (lifecycle.h: masks_changed) and so do the pose-pose Jacobians of its linearisation:
  // keep the masks they were built with for ba_hip_get_pose_pose_leverages
  if (e->mask_version == e->lin_mask_version)
    BAE_HIP(hipMemcpyAsync(e->pose_mask_lin.p, e->pose_mask.p, ((size_t)st.P + st.Pact) * sizeof(uint16_t),
                           hipMemcpyDeviceToDevice, e->stream));
  ++e->mask_version;
  std::vector<uint16_t> m((size_t)st.P + st.Pact, 0);
  for (uint32_t p = 0; p < st.P; ++p) {
    m[p] = by_id[p];
    if (st.pose_opt[p] >= 0) m[st.P + st.pose_opt[p]] = by_id[p];
  }
  BAE_HIP(hipMemcpyAsync(e->pose_mask.p, m.data(), m.size() * sizeof(uint16_t), hipMemcpyHostToDevice,
                         e->stream));
  BAE_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

}  // namespace bae

using namespace bae;

// ===================================================================================
extern "C" {

int ba_hip_create(int lm_dim, int pose_dim, int device, void* stream, ba_hip_engine** out) {
  if (!out) return -1;
  *out = nullptr;
  if (!(lm_dim == 0 || lm_dim == 1 || lm_dim == 3)) return -1;
  if (!(pose_dim == 6 || pose_dim == 9 || pose_dim == 15)) return -1;
  int ndev = 0;
  hipError_t err = hipGetDeviceCount(&ndev);
  if (err != hipSuccess || ndev == 0) return -(int)(err == hipSuccess ? hipErrorNoDevice : err);
  if (device < 0 || device >= ndev) return -(int)hipErrorInvalidDevice;
  err = hipSetDevice(device);
  if (err != hipSuccess) return -(int)err;
  Engine* e = new Engine();
  e->lm_dim = lm_dim; e->pose_dim = pose_dim; e->device = device;
  memset(&e->opt, 0, sizeof(e->opt));
  e->opt.projection_outlier_threshold = 1.0;
  e->opt.use_robust_norm_for_proj_residuals = 1;
  e->opt.use_triangular_matrices = 1;
  e->opt.gyro_sigma = 5.3088444e-5; e->opt.accel_sigma = 0.001883649;
  e->opt.gyro_bias_sigma = 1.4125375e-4; e->opt.accel_bias_sigma = 1.2589254e-2;
  memset(&e->timers, 0, sizeof(e->timers));
  if (stream) {
    e->stream = (hipStream_t)stream;
  } else {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // hi = numerically smallest = highest priority
    err = hipStreamCreateWithPriority(&e->stream, hipStreamDefault, hi);
    if (err != hipSuccess) { delete e; return -(int)err; }
    e->own_stream = true;
  }
  {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    // Second stream for the bulk trailing updates of the factorisation: lowest priority, so the
    // serial panel chain on the main stream wins the dispatch.  (CU masks for it were measured in
    // round 1 — every mask was slower than none.)
    if (!e->stream2) err = hipStreamCreateWithPriority(&e->stream2, hipStreamNonBlocking, lo);
    if (err != hipSuccess) { delete e; return -(int)err; }
  }
  *out = reinterpret_cast<ba_hip_engine*>(e);
  return 0;
}

void ba_hip_destroy(ba_hip_engine* h) {
  if (!h) return;
  Engine* e = reinterpret_cast<Engine*>(h);
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);   // nothing of the engine's in flight when the communicator goes
  comm_release(e);
  delete e;
}

uint64_t ba_hip_device_bytes_live(void) { return (uint64_t)g_device_bytes_live.load(); }

const char* ba_hip_last_error(const ba_hip_engine* h) {
  return h ? reinterpret_cast<const Engine*>(h)->err.c_str() : "null engine";
}

int ba_hip_set_options(ba_hip_engine* h, const ba_hip_options* o) {
  BA_ENTRY_HOST(h);
  e->opt = *o;
  return 0;
}

int ba_hip_set_cameras(ba_hip_engine* h, uint32_t n, const double* params4, const double* t_vs7) {
  BA_ENTRY_HOST(h);
  e->prob.num_cams = n;
  e->prob.cam_params.assign(params4, params4 + 4 * (size_t)n);
  e->prob.cam_tvs.assign(t_vs7, t_vs7 + 7 * (size_t)n);
  e->prob.cam_model.assign(n, 0);
  e->prob.cam_w.assign(n, 0.0);
  e->held.problem_changed();
  return 0;
}

int ba_hip_set_camera_models(ba_hip_engine* h, uint32_t n, const int32_t* model, const double* w) {
  BA_ENTRY_HOST(h);
  if (n != e->prob.num_cams) return e->fail_msg("ba_hip_set_camera_models: one entry per camera of ba_hip_set_cameras expected");
  for (uint32_t c = 0; c < n; ++c) {
    if (model[c] != 0 && model[c] != 1) return e->fail_msg("camera model: 0 (LinearCamera) or 1 (FovCamera)");
    if (model[c] == 1 && !(w && std::isfinite(w[c]))) return e->fail_msg("FovCamera: a finite distortion parameter w is needed");
  }
  e->prob.cam_model.assign(model, model + n);
  e->prob.cam_w.assign(n, 0.0);
  for (uint32_t c = 0; c < n; ++c) if (model[c] == 1) e->prob.cam_w[c] = w[c];
  e->held.problem_changed();
  return 0;
}
int ba_hip_get_camera_fov(ba_hip_engine* h, uint32_t n, double* w) {
  BA_ENTRY_HOST(h);
  if (!w || n != e->prob.cam_w.size()) return e->fail_msg("ba_hip_get_camera_fov: camera count mismatch");
  for (size_t c = 0; c < e->prob.cam_w.size(); ++c) w[c] = e->prob.cam_w[c];
  return 0;
}

int ba_hip_set_pose_cam_params(ba_hip_engine* h, uint32_t n, const double* params4) {
  BA_ENTRY_DEVICE(h);
  e->held.pose_cam_params_changed();
  if (n == 0 || !params4) {
    e->prob.pose_cam_params.clear();
    return 0;
  }
  e->prob.pose_cam_params.assign(params4, params4 + 4 * (size_t)n);
  return upload(e, e->pose_cam, e->prob.pose_cam_params);
}

int ba_hip_set_poses(ba_hip_engine* h, uint32_t n, const double* t_wp7, const double* v_w3,
                     const double* b6, const uint8_t* is_active) {
  BA_ENTRY_HOST(h);
  Problem& pb = e->prob;
  pb.num_poses = n;
  pb.pose_state.assign((size_t)n * kPoseState, 0.0);
  pb.pose_active.assign(n, 1);
  for (uint32_t p = 0; p < n; ++p) {
    double* s = &pb.pose_state[(size_t)p * kPoseState];
    for (int i = 0; i < 7; ++i) s[i] = t_wp7[(size_t)p * 7 + i];
    if (v_w3) for (int i = 0; i < 3; ++i) s[7 + i] = v_w3[(size_t)p * 3 + i];
    if (b6) for (int i = 0; i < 6; ++i) s[10 + i] = b6[(size_t)p * 6 + i];
    if (is_active) pb.pose_active[p] = is_active[p] ? 1 : 0;
  }
  e->held.problem_changed();
  return 0;
}

int ba_hip_set_landmarks(ba_hip_engine* h, uint32_t n, const double* x_w4, const uint32_t* ref_pose_id,
                         const uint32_t* ref_cam_id, const uint8_t* is_active) {
  BA_ENTRY_HOST(h);
  Problem& pb = e->prob;
  pb.num_lms = n;
  pb.lm_xw.assign(x_w4, x_w4 + 4 * (size_t)n);
  pb.lm_ref_pose.assign(ref_pose_id, ref_pose_id + n);
  if (ref_cam_id) pb.lm_ref_cam.assign(ref_cam_id, ref_cam_id + n);
  else pb.lm_ref_cam.assign(n, 0);
  if (is_active) pb.lm_active.assign(is_active, is_active + n);
  else pb.lm_active.assign(n, 1);
  e->held.problem_changed();
  return 0;
}

int ba_hip_set_projection_residuals(ba_hip_engine* h, uint32_t n, const double* z2,
                                    const uint32_t* meas_pose_id, const uint32_t* landmark_id,
                                    const uint32_t* cam_id, const double* weight) {
  BA_ENTRY_HOST(h);
  Problem& pb = e->prob;
  pb.num_proj = n;
  pb.proj_z.assign(z2, z2 + 2 * (size_t)n);
  pb.proj_pose.assign(meas_pose_id, meas_pose_id + n);
  pb.proj_lm.assign(landmark_id, landmark_id + n);
  if (cam_id) pb.proj_cam.assign(cam_id, cam_id + n);
  else pb.proj_cam.assign(n, 0);
  if (weight) pb.proj_w.assign(weight, weight + n);
  else pb.proj_w.assign(n, 1.0);
  e->held.problem_changed();
  return 0;
}

int ba_hip_set_conditioning_residuals(ba_hip_engine* h, uint32_t n, const uint32_t* residual_id) {
  BA_ENTRY_HOST(h);
  e->prob.proj_cond.assign(residual_id, residual_id + n);
  e->held.problem_changed();
  return 0;
}

int ba_hip_set_unary_residuals(ba_hip_engine* h, uint32_t n, const uint32_t* pose_id,
                               const double* t_wp7, const double* cov_inv36,
                               const uint8_t* use_rotation) {
  BA_ENTRY_HOST(h);
  Problem& pb = e->prob;
  pb.num_unary = n;
  pb.un_pose.assign(pose_id, pose_id + n);
  pb.un_t.assign(t_wp7, t_wp7 + 7 * (size_t)n);
  pb.un_cov_inv.assign(cov_inv36, cov_inv36 + 36 * (size_t)n);
  if (use_rotation) pb.un_rot.assign(use_rotation, use_rotation + n);
  else pb.un_rot.assign(n, 1);
  e->held.problem_changed();
  return 0;
}

int ba_hip_set_binary_residuals(ba_hip_engine* h, uint32_t n, const uint32_t* pose1_id,
                                const uint32_t* pose2_id, const double* t_12_7,
                                const double* cov_inv36, const double* cov_inv_sqrt36,
                                const double* weight, const uint8_t* use_rotation) {
  BA_ENTRY_HOST(h);
  Problem& pb = e->prob;
  pb.num_binary = n;
  pb.bin_p1.assign(pose1_id, pose1_id + n);
  pb.bin_p2.assign(pose2_id, pose2_id + n);
  pb.bin_t.assign(t_12_7, t_12_7 + 7 * (size_t)n);
  pb.bin_cov_inv.assign(cov_inv36, cov_inv36 + 36 * (size_t)n);
  pb.bin_cov_inv_sqrt.assign(cov_inv_sqrt36, cov_inv_sqrt36 + 36 * (size_t)n);
  if (weight) pb.bin_w.assign(weight, weight + n);
  else pb.bin_w.assign(n, 1.0);
  if (use_rotation) pb.bin_rot.assign(use_rotation, use_rotation + n);
  else pb.bin_rot.assign(n, 1);
  e->held.problem_changed();
  return 0;
}

int ba_hip_set_imu_residuals(ba_hip_engine* h, uint32_t n, const uint32_t* pose1_id,
                             const uint32_t* pose2_id, const uint32_t* meas_ptr, const double* meas7,
                             const double* weight) {
  BA_ENTRY_HOST(h);
  Problem& pb = e->prob;
  pb.num_imu = n;
  pb.imu_p1.assign(pose1_id, pose1_id + n);
  pb.imu_p2.assign(pose2_id, pose2_id + n);
  pb.imu_ptr.assign(meas_ptr, meas_ptr + n + 1);
  pb.imu_meas.assign(meas7, meas7 + 7 * (size_t)(n ? meas_ptr[n] : 0));
  if (weight) pb.imu_w.assign(weight, weight + n);
  else pb.imu_w.assign(n, 1.0);
  e->held.problem_changed();
  return 0;
}

// Host-side RK4 integration of IMU samples with the code the device kernels use (dpose.h):
// ImuResidualT::IntegrateResidual without Jacobians (Types.h:662-738).
int ba_hip_integrate_imu(const double t_wp7[7], const double v_w3[3], const double bg3[3], const double ba3[3],
                         const double g3[3], const double* meas7, uint32_t nmeas, double* states10) {
  if (!t_wp7 || !v_w3 || !bg3 || !ba3 || !g3 || !states10 || (nmeas && !meas7)) return -1;
  bad::ImuState s;
  for (int i = 0; i < 3; ++i) { s.t[i] = t_wp7[i]; s.v[i] = v_w3[i]; }
  for (int i = 0; i < 4; ++i) s.q[i] = t_wp7[3 + i];
  auto put = [&](uint32_t k) {
    double* o = states10 + 10 * (size_t)k;
    for (int i = 0; i < 3; ++i) { o[i] = s.t[i]; o[7 + i] = s.v[i]; }
    for (int i = 0; i < 4; ++i) o[3 + i] = s.q[i];
  };
  put(0);
  for (uint32_t i = 1; i < nmeas; ++i) {
    s = bad::integrate_imu(s, meas7 + 7 * (size_t)(i - 1), meas7 + 7 * (size_t)i, bg3, ba3, g3, false, nullptr,
                           nullptr, nullptr, nullptr);
    put(i);
  }
  return 0;
}

// The same integration with the Jacobians of the reference's signature (Types.h:662-738): dpose_db
// (10 x 6, over the gyro / accelerometer biases), dpose_dpose (10 x 10, over the start state
// [t q v]) and the covariance c_res (10 x 10, in/out: C <- F C F^T + G R G^T per step) — formed, as in
// the reference, only when one of the two Jacobians is asked for AND the noise diagonal r6 is given.
int ba_hip_integrate_imu_jacobians(const double t_wp7[7], const double v_w3[3], const double bg3[3],
                                   const double ba3[3], const double g3[3], const double* meas7, uint32_t nmeas,
                                   const double r6[6], double* states10, double* dpose_db60,
                                   double* dpose_dpose100, double* c_res100) {
  if (!t_wp7 || !v_w3 || !bg3 || !ba3 || !g3 || !states10 || (nmeas && !meas7)) return -1;
  bad::ImuState s;
  for (int i = 0; i < 3; ++i) { s.t[i] = t_wp7[i]; s.v[i] = v_w3[i]; }
  for (int i = 0; i < 4; ++i) s.q[i] = t_wp7[3 + i];
  auto put = [&](uint32_t k) {
    double* o = states10 + 10 * (size_t)k;
    for (int i = 0; i < 3; ++i) { o[i] = s.t[i]; o[7 + i] = s.v[i]; }
    for (int i = 0; i < 4; ++i) o[3 + i] = s.q[i];
  };
  put(0);
  bad::DM<10, 6> db, dy_db;
  bad::DM<10, 10> dd, dy_dy, cov;
  db.zero();
  dd.identity();
  const bool jac = (dpose_db60 || dpose_dpose100) && r6;
  if (c_res100) for (int i = 0; i < 100; ++i) cov.m[i] = c_res100[i];
  for (uint32_t i = 1; i < nmeas; ++i) {
    const double* z0 = meas7 + 7 * (size_t)(i - 1);
    const double* z1 = meas7 + 7 * (size_t)i;
    if (jac) {
      s = bad::integrate_imu(s, z0, z1, bg3, ba3, g3, true, &dy_db, &dy_dy, c_res100 ? &cov : nullptr, r6);
      db = bad::madd(dy_db, bad::mm(dy_dy, db));  // Types.h:712-714
      dd = bad::mm(dy_dy, dd);                    // Types.h:716-718
    } else {
      s = bad::integrate_imu(s, z0, z1, bg3, ba3, g3, false, nullptr, nullptr, nullptr, nullptr);
    }
    put(i);
  }
  if (dpose_db60) for (int i = 0; i < 60; ++i) dpose_db60[i] = db.m[i];
  if (dpose_dpose100) for (int i = 0; i < 100; ++i) dpose_dpose100[i] = dd.m[i];
  if (c_res100 && jac) for (int i = 0; i < 100; ++i) c_res100[i] = cov.m[i];
  return 0;
}

// ImuResidualT::GetPoseDerivative (Types.h:376-416): k = d/dt [t; rotation vector; v] of the state at
// time z_start.time + dt between two samples, with dk_db (9 x 6) and dk_dx (9 x 10), both optional
int ba_hip_imu_pose_derivative(const double state10[10], const double g3[3], const double z_start7[7],
                               const double z_end7[7], const double bg3[3], const double ba3[3], double dt,
                               double k9[9], double* dk_db54, double* dk_dx90) {
  if (!state10 || !g3 || !z_start7 || !z_end7 || !bg3 || !ba3 || !k9) return -1;
  bad::ImuState s;
  for (int i = 0; i < 3; ++i) { s.t[i] = state10[i]; s.v[i] = state10[7 + i]; }
  for (int i = 0; i < 4; ++i) s.q[i] = state10[3 + i];
  bad::DM<9, 6> a;
  bad::DM<9, 10> b;
  bad::pose_derivative(s, g3, z_start7, z_end7, bg3, ba3, dt, k9, dk_db54 ? &a : nullptr, dk_dx90 ? &b : nullptr);
  if (dk_db54) for (int i = 0; i < 54; ++i) dk_db54[i] = a.m[i];
  if (dk_dx90) for (int i = 0; i < 90; ++i) dk_dx90[i] = b.m[i];
  return 0;
}

// ImuResidualT::IntegratePose (Types.h:324-373): y = state advanced by k * dt (q <- exp(k_w dt) q, not
// renormalised), with dy_dk (10 x 9) and the quaternion block dy_dy (4 x 4), both optional
int ba_hip_imu_integrate_pose(const double state10[10], const double k9[9], double dt, double out10[10],
                              double* dy_dk90, double* dy_dy16) {
  if (!state10 || !k9 || !out10) return -1;
  bad::ImuState s;
  for (int i = 0; i < 3; ++i) { s.t[i] = state10[i]; s.v[i] = state10[7 + i]; }
  for (int i = 0; i < 4; ++i) s.q[i] = state10[3 + i];
  bad::DM<10, 9> a;
  bad::DM<4, 4> b;
  const bad::ImuState y = bad::integrate_pose(s, k9, dt, dy_dk90 ? &a : nullptr, dy_dy16 ? &b : nullptr);
  for (int i = 0; i < 3; ++i) { out10[i] = y.t[i]; out10[7 + i] = y.v[i]; }
  for (int i = 0; i < 4; ++i) out10[3 + i] = y.q[i];
  if (dy_dk90) for (int i = 0; i < 90; ++i) dy_dk90[i] = a.m[i];
  if (dy_dy16) for (int i = 0; i < 16; ++i) dy_dy16[i] = b.m[i];
  return 0;
}

// The Lie-group / quaternion helpers of the reference's Utils.h on the host (include/ba/Utils.h wraps
// them with the reference's names): one dispatcher over the functions the kernels use (dmath.h, dpose.h).
// a / b: the arguments as doubles (transforms as [t(3) q(4)], quaternions x,y,z,w); out: the result,
// row-major.  Returns the number of doubles written, -1 for an unknown op or a missing argument.
int ba_hip_lie(int op, const double* a, const double* b, double* out) {
  using namespace bad;
  if (!a || !out) return -1;
  auto put = [&](const double* m, int n) { for (int i = 0; i < n; ++i) out[i] = m[i]; return n; };
  const bool two = op == 5 || (op >= 7 && op <= 11) || op == 14 || op == 15 || op == 17;
  if (two && !b) return -1;
  switch (op) {
    case 1: return put(dlog_dq(a).m, 12);                                     // Utils.h:137-185
    case 2: return put(dq_exp_dw(v3(a[0], a[1], a[2])).m, 12);                // :252-266
    case 3: return put(qR(a).m, 16);                                          // dq1q2_dq1(q2) :286-291
    case 4: return put(qL(a).m, 16);                                          // dq1q2_dq2(q1) :277-282
    case 5: return put(dqx_dq(a, v3(b[0], b[1], b[2])).m, 12);                // :295-312
    case 6: { const M3 R = quat_to_rot(a[0], a[1], a[2], a[3]); return put(R.m, 9); }  // dqx_dx :316-333
    case 7: log_decoupled(tq_from7(a), tq_from7(b), out); return 6;           // :354-360
    case 8: {                                                                 // exp_decoupled :364-369
      double qe[4], q[4];
      so3_exp(v3(b[3], b[4], b[5]), qe);
      quat_mul(a + 3, qe, q);
      quat_normalize(q);
      for (int i = 0; i < 3; ++i) out[i] = a[i] + b[i];
      for (int i = 0; i < 4; ++i) out[3 + i] = q[i];
      return 7;
    }
    case 9: return put(dlog_decoupled_dx(tq_from7(a), tq_from7(b)).m, 36);    // :374-384
    case 10: return put(dLog_decoupled_dt1(tq_from7(a), tq_from7(b)).m, 42);  // :388-397
    case 11: return put(dlog_decoupled_dt2(tq_from7(a), tq_from7(b)).m, 42);  // :401-447
    case 12: return put(dexp_decoupled_dx(tq_from7(a)).m, 42);                // :451-489
    case 13: return put(dinv_exp_decoupled_dx(tq_from7(a)).m, 42);            // :493-536
    case 14: {                                                                // dt_x_dt(t, x) 4 x 7 :540-583
      double J[28] = {0};
      const DM<3, 4> d = dqx_dq(a + 3, v3(b[0], b[1], b[2]));
      for (int r = 0; r < 3; ++r) {
        J[r * 7 + r] = b[3];
        for (int c = 0; c < 4; ++c) J[r * 7 + 3 + c] = d(r, c);
      }
      return put(J, 28);
    }
    case 15: return put(dt1_t2_dt1(tq_from7(a), tq_from7(b)).m, 49);          // :587-639
    case 16: return put(dt1_t2_dt2(tq_from7(a)).m, 49);                       // :643-694
    case 17: {                                                                // MultHomogeneous :72-82
      const V3 r = qrot(a + 3, v3(b[0], b[1], b[2]));
      out[0] = r.x + a[0] * b[3]; out[1] = r.y + a[1] * b[3]; out[2] = r.z + a[2] * b[3]; out[3] = b[3];
      return 4;
    }
  }
  return -1;
}

int ba_hip_set_imu_noise(ba_hip_engine* h, const double r6[6], const double rb6[6]) {
  BA_ENTRY_HOST(h);
  e->prob.imu_noise.clear();
  if (r6 && rb6) {
    e->prob.imu_noise.assign(r6, r6 + 6);
    e->prob.imu_noise.insert(e->prob.imu_noise.end(), rb6, rb6 + 6);
  }
  return 0;  // not structural: uploaded by the next ba_hip_begin_solve
}

int ba_hip_set_inertial_covariance_once(ba_hip_engine* h, int on, int reset) {
  BA_ENTRY_HOST(h);
  e->imu_cov_once = on != 0;
  if (reset || !on) e->imu_cov_count = 0;
  return 0;
}

int ba_hip_set_gravity(ba_hip_engine* h, const double g3[3]) {
  BA_ENTRY_HOST(h);
  for (int i = 0; i < 3; ++i) e->prob.gravity[i] = g3[i];
  return 0;
}

int ba_hip_finalize(ba_hip_engine* h) {
  BA_ENTRY_DEVICE(h);
  e->held.finalize_begins();
  e->in_solve = false;
  e->resect.list_valid = false;   // the per-pose observation list belongs to the structure built below
  Problem& pb = e->prob;
  if (pb.pose_active.size() != pb.num_poses) pb.pose_active.assign(pb.num_poses, 1);
  if (pb.lm_active.size() != pb.num_lms) pb.lm_active.assign(pb.num_lms, 1);
  if (e->order_mode != kOrderNatural && e->ordering_refused())
    return e->fail_msg("pose ordering is not available on a sharded engine");
  e->opt_of_natural.clear();
  e->group_ptr.clear(); e->group_adj.clear();
  e->order_stats = ba_hip_ordering_stats();
  e->lev_pos.clear();
  e->mask_host.assign(pb.num_poses, 0);
  int rc = build_structure(e);
  if (rc) return rc;
  e->held.finalize_succeeded();
  return 0;
}

int ba_hip_get_conditioning_error(ba_hip_engine* h, double* proj_sq_sum) {
  BA_ENTRY_FINAL(h);
  *proj_sq_sum = 0.0;
  if (e->prob.proj_cond.empty() || e->st.O == 0) return 0;
  int rc = launch_pose_prep(e);
  if (rc) return rc;
  if ((rc = launch_residuals(e, 2))) return rc;
  return sum_partials(e, (e->st.O + 255) / 256, 1, proj_sq_sum);
}

int ba_hip_begin_solve(ba_hip_engine* h) {
  BA_ENTRY_FINAL(h);
  e->held.solve_begins();
  e->in_solve = true;   // until ba_hip_end_solve: x_w lags behind x_s (ba_hip_triangulate_landmarks refuses)
  e->err_cache_off = getenv("BA_HIP_NO_ERR_CACHE") != nullptr;
  if (!e->prob.pose_cam_params.empty() && e->prob.pose_cam_params.size() != 4 * (size_t)e->prob.num_poses)
    return e->fail_msg("per-pose camera parameters: one [fx,fy,u0,v0] per pose expected");
  if (!e->prob.pose_cam_params.empty() && e->has_fov)
    return e->fail_msg("per-pose camera parameters are offered for LinearCamera rigs only");
  int rc = upload_imu_consts(e);
  if (rc) return rc;
  // (calibration: the tables of k_pose_prep keep the T_vs they were last built with across Solve()
  // calls — after a Solve() that ended in a rejected step the reference's poses carry their cached
  // T_sw of the T_vs before that step into the next call, until a step is applied: tvs_eval is not
  // resynchronised with the rig here)
  rc = launch_pose_prep(e);
  if (rc) return rc;
  rc = launch_begin_solve(e);
  if (rc) return rc;
  BAE_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

int ba_hip_set_pose_masks(ba_hip_engine* h, uint32_t n, const uint16_t* masks) {
  BA_ENTRY_FINAL(h);
  if (n != e->st.P) return e->fail_msg("mask count != pose count");
  e->held.masks_changed();
  e->mask_host.assign(masks, masks + n);
  return set_masks_device(e, std::vector<uint16_t>(masks, masks + n));
}

int ba_hip_linearize(ba_hip_engine* h, ba_hip_errors* out) {
  BA_ENTRY_FINAL(h);
  const Structure& st = e->st;
  ba_hip_errors errs = {0, 0, 0, 0};
  int rc;
  if (e->damp.lambda_next > 0.0) BA_ASK(damping_refusal(e));
  e->held.linearize_begins();
  e->damp.lambda_lin = e->damp.lambda_next;   // the rows, V^-1 and S written below are those of H + lambda D
  e->damp.terms_valid = false;
  e->damp.poses_ms = e->damp.terms_ms = 0.0;
  if ((rc = damp_prepare(e))) return rc;
  // projection errors at the linearisation point -> Huber sigma
  EventTimer t_j(e);
  if ((rc = launch_pose_prep(e))) return rc;
  // the errors of the Huber median: left by the last EvaluateResiduals at this state, or computed now
  const bool cached = e->err_cache_on() && e->held.obs_e_valid[e->cur] && e->obs_e_state[e->cur].n >= st.O && st.O > 0;
  const double* med_in = cached ? e->obs_e_state[e->cur].p : e->obs_e.p;
  if (!cached && (rc = launch_residuals(e, 0))) return rc;
  t_j.mark();
  EventTimer t_r(e);
  double c_huber = 0.0;
  uint64_t n_total = st.O;
  if (e->sharded()) {
    double cnt = (double)st.O;
    BAE_HIP(hipMemcpy(e->scalars_out.p, &cnt, sizeof(double), hipMemcpyHostToDevice));
    if (shard_allreduce(e, e->scalars_out.p, 1, 0) != 0) return e->fail_msg("allreduce hook failed");
    BAE_HIP(hipMemcpy(&cnt, e->scalars_out.p, sizeof(double), hipMemcpyDeviceToHost));
    n_total = (uint64_t)(cnt + 0.5);
  }
  if (n_total > 0) {
    double med = 0.0;
    // std::nth_element at floor(N * 0.5): the upper median (BundleAdjuster.cpp:1356-1358)
    if ((rc = select_kth(e, med_in, st.O, (uint64_t)std::floor(n_total * 0.5), &med))) return rc;
    c_huber = 1.2107 * std::sqrt(med);
  }
  t_r.mark();
  // The inertial kernels run on the second stream.  Sliding windows (few samples: latency-bound wavefront forms)
  // start them right away, beside the projection linearisation.  Large problems start them BEHIND k_linearize, under
  // the tile assembly: the lane-per-sample form keeps 28 KB of private memory per lane, and its scratch traffic beside
  // the bandwidth-bound k_linearize slowed that kernel 4-5x (configs[4]: 3.8-5.6 ms against 1.05 ms alone) for the
  // same wall time (profiles/r03_imu_ab.txt); the assembly is latency-bound on its row gathers
  // and four times as long as both inertial passes.
  const bool imu_late = e->prob.imu_meas.size() / 7 > 4096;
  if (!imu_late && (rc = launch_imu_early(e, c_huber))) return rc;
  EventTimer t_l(e);
  // from here on every sum stays on the device until ONE copy at the end of the call (sums.flush()): the
  // assembly and the pose-pose kernels are enqueued without waiting for the linearisation to finish
  double* hs = e->eval_h;  // proj | unary | binary | inertial
  for (int i = 0; i < 4; ++i) hs[i] = 0.0;
  DeferScope sums(e);
  if ((rc = launch_landmarks(e, c_huber, e->opt.use_robust_norm_for_proj_residuals))) return rc;
  if (imu_late && (rc = launch_imu_early(e, c_huber))) return rc;
  // proj_error_ of BuildProblem (BundleAdjuster.cpp:1386): sum of w |r|^2 with the new weights, one
  // partial per linearisation wave
  if ((rc = sum_partials(e, st.O ? st.n_chunks : 0, 1, hs))) return rc;
  t_l.mark();
  EventTimer t_s(e);
  e->held.linearize_writes_A();
  e->lin_mask_version = e->mask_version;   // the rows above and the system about to be gathered carry the current masks
  if ((rc = launch_gather_S(e)) || (rc = launch_posepose_build(e, c_huber, hs + 1))) return rc;
  // dense priors after k_pp_scatter, in prior order; their E_p is folded into unary_error
  if ((rc = launch_priors(e, 1, &e->prior_err_h))) return rc;
  // A holds the complete S: the pose part of the damping, before anything reads or copies it
  std::unique_ptr<EventTimer> t_d;
  if (e->damp.lambda_lin > 0.0) {
    t_d.reset(new EventTimer(e));
    if ((rc = launch_damp_poses(e))) return rc;
    t_d->mark();
  }
  if (e->prob.num_unary + e->prob.num_binary + e->prob.num_imu)  // kept for ba_hip_marginalize (the dogleg reuses pp_err)
    BAE_HIP(hipMemcpyAsync(e->pp_err_lin.p, e->pp_err.p, (size_t)(e->prob.num_unary + e->prob.num_binary + e->prob.num_imu) *
                           sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  // copy the reduced rhs into the rhs row of A
  BAE_HIP(hipMemcpyAsync(e->A.p + (size_t)st.ld * st.ld, e->rhs_sc.p, (size_t)st.n * sizeof(double),
                         hipMemcpyDeviceToDevice, e->stream));
  if (e->sharded()) {
    // S (lower storage) with its rhs row, and the unreduced rhs_p, are sums over the
    // landmark shards: one all-reduce each over xGMI.
    if (dist_solve_enabled(e)) {
      // distributed reduced solve: every rank only needs the sum of the column panels it owns
      // (reduce-scatter); the reduced rhs (one row) and rhs_p are summed everywhere
      BAE_HIP(hipStreamSynchronize(e->stream));
      // the union tile pattern decides which tiles of S travel (a collective on first use)
      if (!e->held.nzL_valid && (rc = factor_tile_pattern(e))) return rc;
      if (shard_allreduce(e, e->rhs_sc.p, st.ld, 0) != 0) return e->fail_msg("allreduce hook failed");
      if (shard_allreduce(e, e->rhs_p.p, st.ld, 0) != 0) return e->fail_msg("allreduce hook failed");
      if ((rc = dist_reduce_scatter_S(e))) return rc;
      BAE_HIP(hipMemcpyAsync(e->A.p + (size_t)st.ld * st.ld, e->rhs_sc.p, (size_t)st.n * sizeof(double),
                             hipMemcpyDeviceToDevice, e->stream));
    } else {
    // The message is the packed lower triangle + rhs row (half of the square storage).
    const size_t cnt = packed_lower_count(st.ld);
    BAE_HIP(e->packed.alloc(cnt));
    if ((rc = launch_pack_lower(e, 0))) return rc;
    BAE_HIP(hipStreamSynchronize(e->stream));
    if (shard_allreduce(e, e->packed.p, cnt, 0) != 0)
      return e->fail_msg("allreduce hook failed");
    if ((rc = launch_pack_lower(e, 1))) return rc;
    if (shard_allreduce(e, e->rhs_p.p, st.ld, 0) != 0)
      return e->fail_msg("allreduce hook failed");
    BAE_HIP(hipMemcpyAsync(e->rhs_sc.p, e->A.p + (size_t)st.ld * st.ld, (size_t)st.n * sizeof(double),
                           hipMemcpyDeviceToDevice, e->stream));
    }
  }
  t_s.mark();
  if ((rc = sums.flush())) return rc;
  e->timers.j_evaluation = t_j.read_ms() + t_l.read_ms();
  e->timers.robust_weights = t_r.read_ms();
  e->timers.jtj_schur = t_s.read_ms();
  if (t_d) e->damp.poses_ms = t_d->read_ms();
  errs.proj_error = hs[0]; errs.unary_error = hs[1] + e->prior_err_h; errs.binary_error = hs[2]; errs.inertial_error = hs[3];
  e->held.linearize_succeeded();
  if (out) *out = errs;
  return 0;
}

int ba_hip_solve_gn(ba_hip_engine* h) {
  BA_ENTRY_FINAL(h);
  const Structure& st = e->st;
  int status = 0, rc;
  EventTimer t(e);
  // CalculateGn runs only with active poses (BundleAdjuster.cpp:959-964, 1089-1094): with none, the
  // calibration unknowns are not solved for either (delta_k stays empty in the reference)
  const bool skip = st.K && st.Pact == 0;
  e->held.gn_solve_begins();
  if (skip) BAE_HIP(hipMemsetAsync(e->gn_p.p, 0, e->gn_p.bytes(), e->stream));
  if (st.n > 0 && !skip && e->solver_mode == BA_HIP_SOLVER_PCG) {
    // S stays in A: no factor, no kept copy
    if (e->pcg_refused()) return e->fail_msg("the PCG solver is not available on a sharded engine");
    if (!e->held.nzL_valid && (rc = factor_tile_pattern(e))) return rc;
    const bool rebuild = e->pcg_plan_version != e->nzL_version || e->pcg_plan.nt != st.ld / 64 || e->pcg_blk.size() != (size_t)2 * st.ld;
    if (rebuild) {
      build_pcg_plan(e->nzS_host, st.ld / 64, e->pcg_plan);
      pcg_row_blocks(st.np, (uint32_t)e->pose_dim, st.K, st.ld, e->pcg_blk, e->pcg_blocks);
      e->pcg_plan_version = e->nzL_version;
      e->pcg_coarse_built = 0;
    }
    if (e->pcg_opt.coarse_aggregate && e->pcg_coarse_built != e->pcg_opt.coarse_aggregate) {
      // aggregates of consecutive active poses in pose-id order; pose_opt says where a pose ordering put their rows
      const uint32_t D = (uint32_t)e->pose_dim;
      std::vector<uint32_t> nat(st.ld, kPcgNone);
      uint32_t a = 0;
      for (uint32_t p = 0; p < st.P; ++p)
        if (st.pose_opt[p] >= 0) {
          for (uint32_t d = 0; d < D; ++d) nat[(size_t)st.pose_opt[p] * D + d] = a * D + d;
          ++a;
        }
      for (uint32_t k = 0; k < st.K; ++k) nat[st.np + k] = st.Pact * D + k;
      build_pcg_coarse(e->pcg_plan, nat, st.Pact, D, st.K, e->pcg_opt.coarse_aggregate);
      e->pcg_coarse_built = e->pcg_opt.coarse_aggregate;
    }
    if ((rc = pcg_solve_device(e, e->A.p, st.n, st.ld, e->rhs_sc.p, e->pcg_plan, e->nzS_host, e->pcg_blk, e->pcg_blocks, rebuild,
                               e->pcg_opt, e->gn_p.p, &e->pcg_stats, &status))) return rc;
    e->held.solved_by_pcg();
  } else if (st.n > 0 && !skip) {
    if (e->opt.keep_reduced_system) {
      BAE_HIP(e->A_keep.alloc((size_t)st.ld * st.ld));
      BAE_HIP(hipMemcpyAsync(e->A_keep.p, e->A.p, (size_t)st.ld * st.ld * sizeof(double),
                             hipMemcpyDeviceToDevice, e->stream));
    }
    if (!e->held.nzL_valid && (rc = factor_tile_pattern(e))) return rc;
    if (dist_solve_enabled(e)) {
      if ((rc = cholesky_solve_dist(e, e->A.p, st.ld, e->gn_p.p, &status, e->nzL.p))) return rc;
    } else {
      const uint32_t nt = st.ld / 64;
      const bool pat = e->nzL_host.size() == (size_t)nt * nt;
      if ((rc = ensure_bulk_lists(e, nt, pat ? e->nzL_host.data() : nullptr, e->nzL_version, &e->bulk_lists))) return rc;
      if ((rc = cholesky_solve(e, e->A.p, st.n, st.ld, e->gn_p.p, &status, e->nzL.p, &e->bulk_lists))) return rc;
    }
    e->held.solved_directly();
  }
  e->timers.solve = t.stop_ms();
  EventTimer tb(e);
  if ((rc = launch_backsub(e))) return rc;
  e->timers.back_substitution = tb.stop_ms();
  e->damp.terms_valid = false;
  if (e->damp.lambda_lin > 0.0 && !status) {
    EventTimer td(e);
    if ((rc = launch_damp_terms(e))) return rc;
    e->damp.terms_ms = td.stop_ms();
  }
  return status ? BA_HIP_FACTORIZATION_ERROR : 0;
}

int ba_hip_dogleg_terms(ba_hip_engine* h, int gn_available, ba_hip_dogleg_scalars* out) {
  BA_ENTRY_FINAL(h);
  if (e->damp.lambda_lin > 0.0)
    return e->fail_msg("ba_hip_dogleg_terms: the linearisation the device holds is damped (ba_hip_set_damping); the dogleg "
                       "step is not combined with damping");
  // every sum of this call stays on the device until ONE copy at the end (sums.flush())
  memset(out, 0, sizeof(*out));
  double* dh = e->dog_h;
  // the steepest-descent denominator |J rhs|^2 does not involve the Gauss-Newton step: the second call of
  // an iteration (gn_available, BundleAdjuster.cpp:971-1002) reuses what the first one summed
  const bool reuse = gn_available && e->held.dog_jrhs_valid;
  DeferScope sums(e);
  int rc = launch_dogleg(e, gn_available, dh, reuse);
  if (!rc && !reuse) rc = launch_posepose_jrhs(e, dh + 7);
  if (!rc && !reuse) rc = launch_priors_jrhs(e, &e->prior_jrhs_h);
  if (!rc) rc = sums.flush();
  e->held.dogleg_sums(!rc);
  if (rc) return rc;
  out->rhs_p_sq = dh[0]; out->gn_p_sq = dh[1]; out->rhs_gn_p = dh[2];
  out->rhs_l_sq = dh[3]; out->gn_l_sq = dh[4]; out->rhs_gn_l = dh[5];
  out->j_rhs_sq = dh[6] + dh[7] + e->prior_jrhs_h;
  return e->st.K ? launch_calib_dogleg(e, gn_available, out) : 0;
}

// ---- Levenberg-Marquardt damping (damping.h, k_damp.hip) ----------------------------------------------------------
int ba_hip_set_damping(ba_hip_engine* h, double lambda) {
  BA_ENTRY_HOST(h);
  if (!(lambda >= 0.0) || !std::isfinite(lambda)) return e->fail_msg("ba_hip_set_damping: lambda must be finite and >= 0");
  if (lambda > 0.0) BA_ASK(damping_refusal(e));
  e->damp.lambda_next = lambda;
  return 0;
}

int ba_hip_damping_update(ba_hip_engine* h, double* lambda, double* nu, double rho) {
  BA_ENTRY_HOST(h);
  if (!lambda || !nu) return e->fail_msg("ba_hip_damping_update: NULL argument");
  DampState s = {*lambda, *nu};
  const bool accepted = damp_update(&s, rho);
  *lambda = s.lambda;
  *nu = s.nu;
  return accepted ? 1 : 0;
}

int ba_hip_get_damping_terms(ba_hip_engine* h, ba_hip_damping_terms* out) {
  BA_ENTRY_FINAL(h);
  if (!out) return e->fail_msg("ba_hip_get_damping_terms: NULL argument");
  memset(out, 0, sizeof(*out));
  out->lambda = e->damp.lambda_lin;
  if (!(e->damp.lambda_lin > 0.0)) return 0;
  if (!e->damp.terms_valid)
    return e->fail_msg("ba_hip_get_damping_terms: needs a finished ba_hip_solve_gn of the damped linearisation");
  const double* t = e->damp.terms_h;
  out->predicted_decrease = t[0]; out->step_scaled_sq = t[1];
  out->diag_min = t[2]; out->diag_max = t[3];
  out->device_ms = e->damp.poses_ms + e->damp.terms_ms;
  return 0;
}

int ba_hip_get_damping_diagonal(ba_hip_engine* h, double* d_p, double* d_l) {
  BA_ENTRY_FINAL(h);
  const Structure& st = e->st;
  if (!(e->damp.lambda_lin > 0.0))
    return e->fail_msg("ba_hip_get_damping_diagonal: the linearisation the device holds is not damped (ba_hip_set_damping)");
  BAE_HIP(hipStreamSynchronize(e->stream));
  if (d_p && st.np) BAE_HIP(hipMemcpy(d_p, e->damp.d_p.p, (size_t)st.np * 8, hipMemcpyDeviceToHost));
  unpermute_vec(e, st.np ? d_p : nullptr);
  if (d_l && st.Lact) {
    std::vector<double> dl((size_t)st.L * e->lm_dim);
    BAE_HIP(hipMemcpy(dl.data(), e->damp.d_l.p, dl.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t l = 0; l < st.L; ++l)
      if (st.lm_opt[l] >= 0)
        for (int k = 0; k < e->lm_dim; ++k) d_l[(size_t)st.lm_opt[l] * e->lm_dim + k] = dl[(size_t)l * e->lm_dim + k];
  }
  return 0;
}

int ba_hip_compose_step(ba_hip_engine* h, double coef_rhs, double coef_gn, ba_hip_step_norms* out) {
  BA_ENTRY_FINAL(h);
  double n2[2];
  DeferScope sums(e);  // both norms in one copy; declared after n2, which the reductions register
  int rc = launch_compose_step(e, coef_rhs, coef_gn, n2);
  if (!rc) rc = sums.flush();
  if (rc) return rc;
  if (out) { out->step_p_norm = std::sqrt(n2[0]); out->step_l_norm = std::sqrt(n2[1]); }
  return 0;
}

int ba_hip_apply_step(ba_hip_engine* h) {
  BA_ENTRY_FINAL(h);
  EventTimer t(e);
  int rc = launch_apply_step(e);
  if (rc) return rc;
  e->cur = 1 - e->cur;
  e->held.step_applied(e->cur);
  if (e->calib_dim && !e->calib_tvs && e->st.C > 0) {
    // BundleAdjuster.cpp:46-69: params of camera 0 -= delta_k, then every x_s ray is re-derived from
    // the landmark's reference pixel with the new parameters, keeping its length
    double dk[5] = {0, 0, 0, 0, 0};
    BAE_HIP(hipMemcpyAsync(dk, e->step_p.p + e->st.np, e->st.K * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    BAE_HIP(hipStreamSynchronize(e->stream));
    e->cam_params_prev = e->prob.cam_params;
    e->cam_w_prev = e->prob.cam_w;
    for (int i = 0; i < 4; ++i) e->prob.cam_params[i] -= dk[i];
    if (e->st.K == 5) e->prob.cam_w[0] -= dk[4];
    if ((rc = upload_cameras(e, false))) return rc;
    if ((rc = launch_reset_rays(e))) return rc;
  }
  if (e->calib_tvs && e->st.C > 0) {
    // BundleAdjuster.cpp:72-83: T_vs of camera 0 <- exp_decoupled(T_vs, -delta_k); the step's tail
    // is delta_k.  The pose caches are rebuilt from the new rig below (t_sw.clear(), :114).
    double dk[6];
    BAE_HIP(hipMemcpyAsync(dk, e->step_p.p + e->st.np, sizeof(dk), hipMemcpyDeviceToHost, e->stream));
    BAE_HIP(hipStreamSynchronize(e->stream));
    double* t = e->prob.cam_tvs.data();
    for (int i = 0; i < 3; ++i) t[i] -= dk[i];
    double qe[4], q[4];
    bad::so3_exp(bad::v3(-dk[3], -dk[4], -dk[5]), qe);
    bad::quat_mul(t + 3, qe, q);
    bad::quat_normalize(q);
    for (int i = 0; i < 4; ++i) t[3 + i] = q[i];
    e->tvs_eval_prev = e->tvs_eval;
    e->tvs_eval = e->prob.cam_tvs;
    if ((rc = upload_cameras(e, false))) return rc;
  }
  rc = launch_pose_prep(e);
  if (rc) return rc;
  e->timers.apply_update = t.stop_ms();
  return 0;
}

int ba_hip_rollback(ba_hip_engine* h) {
  BA_ENTRY_FINAL(h);
  if (!e->held.has_snapshot) return e->fail_msg("no snapshot to roll back to");
  e->cur = 1 - e->cur;
  e->held.rolled_back();
  int rc;
  if (e->calib_tvs) {
    // the reference restores the poses WITH their cached T_sw but not the rig (:1060-1068): the
    // tables go back to the T_vs they were built with, `cam` keeps the rejected update
    e->tvs_eval = e->tvs_eval_prev;
    if ((rc = upload_cameras(e, true))) return rc;
  } else if (e->calib_dim) {
    // the intrinsics ARE restored (params_backup, :1066, :1147); the rays come back with the landmark buffer
    e->prob.cam_params = e->cam_params_prev;
    e->prob.cam_w = e->cam_w_prev;
    if ((rc = upload_cameras(e, false))) return rc;
  }
  rc = launch_pose_prep(e);
  if (rc) return rc;
  BAE_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

int ba_hip_eval_residuals(ba_hip_engine* h, ba_hip_errors* out) {
  BA_ENTRY_FINAL(h);
  ba_hip_errors errs = {0, 0, 0, 0};
  EventTimer t(e);
  double* hs = e->eval_h;  // proj | unary | binary | inertial: one copy for the four sums (sums.flush())
  for (int i = 0; i < 4; ++i) hs[i] = 0.0;
  DeferScope sums(e);
  int rc = launch_residuals(e, 1);
  if (!rc) rc = sum_partials(e, (e->st.O + 255) / 256, 1, hs);
  if (!rc) rc = launch_posepose_eval(e, hs + 1);
  if (!rc) rc = launch_priors(e, 0, &e->prior_err_h);
  if (!rc) rc = sums.flush();
  if (rc) return rc;
  errs.proj_error = hs[0]; errs.unary_error = hs[1] + e->prior_err_h; errs.binary_error = hs[2]; errs.inertial_error = hs[3];
  e->timers.evaluate_residuals = t.stop_ms();
  if (out) *out = errs;
  return 0;
}

int ba_hip_end_solve(ba_hip_engine* h) {
  BA_ENTRY_FINAL(h);
  int rc = launch_end_solve(e);
  if (rc) return rc;
  BAE_HIP(hipStreamSynchronize(e->stream));
  e->in_solve = false;
  return 0;
}

// ---- results --------------------------------------------------------------------------
int ba_hip_get_poses(ba_hip_engine* h, double* t_wp7, double* v_w3, double* b6) {
  BA_ENTRY_FINAL(h);
  const uint32_t P = e->st.P;
  std::vector<double> s((size_t)P * kPoseState);
  BAE_HIP(hipStreamSynchronize(e->stream));
  if (P) BAE_HIP(hipMemcpy(s.data(), e->pose_state[e->cur].p, s.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (uint32_t p = 0; p < P; ++p) {
    const double* r = &s[(size_t)p * kPoseState];
    if (t_wp7) for (int i = 0; i < 7; ++i) t_wp7[(size_t)p * 7 + i] = r[i];
    if (v_w3) for (int i = 0; i < 3; ++i) v_w3[(size_t)p * 3 + i] = r[7 + i];
    if (b6) for (int i = 0; i < 6; ++i) b6[(size_t)p * 6 + i] = r[10 + i];
  }
  return 0;
}

int ba_hip_get_landmarks(ba_hip_engine* h, double* x_w4) {
  BA_ENTRY_FINAL(h);
  BAE_HIP(hipStreamSynchronize(e->stream));
  const double* src = e->lm_dim == 1 ? e->lm_xw.p : e->lm_x[e->cur].p;
  if (e->st.L) BAE_HIP(hipMemcpy(x_w4, src, (size_t)e->st.L * 4 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int ba_hip_get_landmark_flags(ba_hip_engine* h, uint8_t* is_reliable, uint32_t* num_outliers) {
  BA_ENTRY_FINAL(h);
  BAE_HIP(hipStreamSynchronize(e->stream));
  if (e->st.L && is_reliable)
    BAE_HIP(hipMemcpy(is_reliable, e->lm_reliable[e->cur].p, e->st.L, hipMemcpyDeviceToHost));
  if (e->st.L && num_outliers)
    BAE_HIP(hipMemcpy(num_outliers, e->lm_outliers.p, (size_t)e->st.L * 4, hipMemcpyDeviceToHost));
  return 0;
}

uint32_t ba_hip_num_pose_params(const ba_hip_engine* h) {
  return reinterpret_cast<const Engine*>(h)->st.np;
}
uint32_t ba_hip_num_calib_params(const ba_hip_engine* h) {
  return reinterpret_cast<const Engine*>(h)->st.K;
}
int ba_hip_set_calibration(ba_hip_engine* h, int calib_size, int do_tvs) {
  BA_ENTRY_HOST(h);
  if (calib_size != 0 && calib_size != 4 && calib_size != 5)
    return e->fail_msg("CalibSize must be 0, 4 (LinearCamera: fx, fy, u0, v0) or 5 (FovCamera: fx, fy, u0, v0, w)");
  if (calib_size && do_tvs)
    return e->fail_msg("CalibSize > 0 together with DoTvs is not offered: the reference's T_vs block wipes the intrinsics "
                       "columns it shares an entry with (BundleAdjuster.cpp:1775-1783)");
  if ((do_tvs || calib_size) && e->lm_dim != 1)
    return e->fail_msg("calibration columns need LmSize 1 (parallel_algos.h:102-131)");
  if ((do_tvs || calib_size) && e->damp.lambda_next > 0.0)
    return e->fail_msg("ba_hip_set_calibration: damping is set (ba_hip_set_damping) and is not offered with calibration unknowns");
  e->calib_dim = do_tvs ? 6 : calib_size;
  e->calib_tvs = do_tvs != 0;
  e->held.calibration_changed();
  return 0;
}
int ba_hip_get_calibration_marginals(ba_hip_engine* h, double* cov) {
  BA_ENTRY_FINAL(h);
  if (!e->st.K) return e->fail_msg("no calibration columns (ba_hip_set_calibration)");
  BA_ASK(guard_kept_factor(e->held, guard_facts(e), "ba_hip_get_calibration_marginals", nullptr, false));
  return trailing_marginals(e, e->A.p, e->st.ld, e->st.np, e->st.K, cov);
}
int ba_hip_set_landmark_ref_pixels(ba_hip_engine* h, uint32_t n, const double* z_ref2) {
  BA_ENTRY_HOST(h);
  e->prob.lm_zref.assign(z_ref2, z_ref2 + 2 * (size_t)n);
  e->held.problem_changed();
  return 0;
}
int ba_hip_get_camera_params(ba_hip_engine* h, uint32_t n, double* params4) {
  BA_ENTRY_HOST(h);
  const std::vector<double>& p = e->prob.cam_params;
  if (!params4 || (size_t)n * 4 != p.size()) return e->fail_msg("ba_hip_get_camera_params: camera count mismatch");
  for (size_t i = 0; i < p.size(); ++i) params4[i] = p[i];
  return 0;
}
int ba_hip_get_cameras(ba_hip_engine* h, uint32_t n, double* t_vs7) {
  BA_ENTRY_HOST(h);
  const std::vector<double>& t = e->prob.cam_tvs;
  if (!t_vs7 || (size_t)n * 7 != t.size()) return e->fail_msg("ba_hip_get_cameras: camera count mismatch");
  for (size_t i = 0; i < t.size(); ++i) t_vs7[i] = t[i];
  return 0;
}
uint32_t ba_hip_num_lm_params(const ba_hip_engine* h) {
  const Engine* e = reinterpret_cast<const Engine*>(h);
  return e->st.Lact * e->lm_dim;
}

int ba_hip_get_S(ba_hip_engine* h, double* s_nxn) {
  BA_ENTRY_FINAL(h);
  const Structure& st = e->st;
  const uint32_t n = st.n, ld = st.ld, D = e->pose_dim;
  const StructureView sv = structure_view(e);
  auto block_of = [&](uint32_t r) { return r < st.np ? r / D : st.Pact; };  // the calibration border is one more block
  std::vector<double> a((size_t)n * ld);
  BAE_HIP(hipStreamSynchronize(e->stream));
  BA_ASK(guard_get_S(e->held, guard_facts(e)));
  const double* src = e->held.factored ? e->A_keep.p : e->A.p;
  if (n) BAE_HIP(hipMemcpy(a.data(), src, a.size() * sizeof(double), hipMemcpyDeviceToHost));
  // lower storage -> the reference's s_: block (i,j) kept for i <= j only when
  // use_triangular_matrices (SparseBlockMatrixOps.h:236-238), full symmetric otherwise
  // (r, c) in the caller's numbering, (ri, ci) in the engine's; the triangle kept is the caller's
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = 0; c < n; ++c) {
      const uint32_t ri = int_row(sv, r), ci = int_row(sv, c);
      const uint32_t bi = block_of(ri), bj = block_of(ci);
      double v;
      if (bi == bj) v = a[(size_t)ri * ld + ci];
      else if (bi < bj) v = a[(size_t)ci * ld + ri];
      else v = a[(size_t)ri * ld + ci];
      if (e->opt.use_triangular_matrices && block_of(r) > block_of(c)) v = 0.0;
      s_nxn[(size_t)r * n + c] = v;
    }
  return 0;
}

int ba_hip_set_pose_permutation(ba_hip_engine* h, const uint32_t* opt_of_natural, uint32_t n) {
  BA_ENTRY_HOST(h);
  if (n && !opt_of_natural) return e->fail_msg("ba_hip_set_pose_permutation: NULL permutation");
  e->order_user.assign(opt_of_natural, opt_of_natural + n);
  return 0;
}

int ba_hip_get_pose_ordering(ba_hip_engine* h, uint32_t* opt_of_natural, ba_hip_ordering_stats* out) {
  BA_ENTRY_HOST(h);
  if (!e->held.finalized) return e->fail_msg(kNotFinalized);
  if (opt_of_natural)
    for (uint32_t i = 0; i < e->st.Pact; ++i) opt_of_natural[i] = e->opt_of_natural.empty() ? i : e->opt_of_natural[i];
  if (out) *out = e->order_stats;
  return 0;
}

int ba_hip_get_pose_group_graph(ba_hip_engine* h, uint32_t* ptr, uint32_t* adj, uint32_t* num_groups, uint32_t* num_edges) {
  BA_ENTRY_HOST(h);
  if (!e->held.finalized) return e->fail_msg(kNotFinalized);
  const uint32_t ng = e->group_ptr.empty() ? 0 : (uint32_t)e->group_ptr.size() - 1;
  if (num_groups) *num_groups = ng;
  if (num_edges) *num_edges = (uint32_t)e->group_adj.size();
  if (ptr && !e->group_ptr.empty()) memcpy(ptr, e->group_ptr.data(), e->group_ptr.size() * 4);
  if (adj && !e->group_adj.empty()) memcpy(adj, e->group_adj.data(), e->group_adj.size() * 4);
  return 0;
}

int ba_hip_set_collectives(ba_hip_engine* h, ba_hip_collective_fn fn, void* ctx) {
  BA_ENTRY_HOST(h);
  if (fn && e->order_mode != kOrderNatural)
    return e->fail_msg("the collectives hook needs natural pose order (ba_hip_set_pose_ordering is set)");
  if (fn && e->solver_mode == BA_HIP_SOLVER_PCG)
    return e->fail_msg("the collectives hook needs the direct reduced solver (ba_hip_set_reduced_solver selected PCG)");
  e->coll = fn; e->coll_ctx = ctx;
  e->dist.key = ~0ull;
  return 0;
}

int ba_hip_set_allreduce(ba_hip_engine* h, ba_hip_allreduce_fn fn, void* ctx, int rank, int nranks) {
  BA_ENTRY_HOST(h);
  if (fn && e->order_mode != kOrderNatural)
    return e->fail_msg("the all-reduce hook needs natural pose order (ba_hip_set_pose_ordering is set)");
  if (fn && e->solver_mode == BA_HIP_SOLVER_PCG)
    return e->fail_msg("the all-reduce hook needs the direct reduced solver (ba_hip_set_reduced_solver selected PCG)");
  e->allreduce = fn; e->allreduce_ctx = ctx; e->rank = rank; e->nranks = nranks < 1 ? 1 : nranks;
  e->sharding_changed();
  return 0;
}

// ---- dense pose priors and marginalisation (k_marg.hip, marg.h) --------------------------------------
int ba_hip_set_dense_priors(ba_hip_engine* h, uint32_t n, const uint32_t* ptr, const uint32_t* pose_ids,
                            const double* x0_16, const double* H, const double* b, const double* c) {
  BA_ENTRY_HOST(h);
  const int D = e->pose_dim;
  if (n && (!ptr || !pose_ids || !x0_16 || !H || !b || !c)) return e->fail_msg("ba_hip_set_dense_priors: NULL argument");
  if (n == 0) {  // removes the priors
    e->dpri = DensePriors();
    e->held.problem_changed();
    return 0;
  }
  if (ptr[0] != 0) return e->fail_msg("ba_hip_set_dense_priors: ptr[0] must be 0");
  for (uint32_t q = 0; q < n; ++q)
    if (ptr[q + 1] <= ptr[q]) return e->fail_msg("ba_hip_set_dense_priors: every prior needs at least one pose");
  DensePriors pr;
  pr.ptr.assign(ptr, ptr + n + 1);
  const uint32_t ktot = pr.ptr.back();
  for (uint32_t q = 0; q < n; ++q)
    if ((uint64_t)(ptr[q + 1] - ptr[q]) * D > kMargMaxB)
      return e->fail_msg("ba_hip_set_dense_priors: a prior exceeds 4096 unknowns");
  pr.pose.assign(pose_ids, pose_ids + ktot);
  pr.x0.assign(x0_16, x0_16 + (size_t)ktot * kPoseState);
  pr.offsets(D);
  pr.H.assign(H, H + pr.h_off[n]);
  // E_p only sees the symmetric part of H: keep (H + H^T) / 2 (a symmetric H is kept bit for bit)
  for (uint32_t q = 0; q < n; ++q) {
    const size_t kD = (size_t)(pr.ptr[q + 1] - pr.ptr[q]) * D;
    double* h = pr.H.data() + pr.h_off[q];
    for (size_t r = 0; r < kD; ++r)
      for (size_t c = 0; c < r; ++c) h[r * kD + c] = h[c * kD + r] = 0.5 * (h[r * kD + c] + h[c * kD + r]);
  }
  pr.b.assign(b, b + (size_t)ktot * D);
  pr.c.assign(c, c + n);
  e->dpri = std::move(pr);
  e->held.problem_changed();
  return 0;
}

int ba_hip_get_prior_errors(ba_hip_engine* h, uint32_t n, double* out) {
  BA_ENTRY_FINAL(h);
  if (n != e->dpri.count() || (n && !out)) return e->fail_msg("ba_hip_get_prior_errors: one entry per dense prior expected");
  if (!n) return 0;
  BAE_HIP(hipStreamSynchronize(e->stream));
  if (!e->dp_E_last) { for (uint32_t q = 0; q < n; ++q) out[q] = 0.0; return 0; }
  BAE_HIP(hipMemcpy(out, e->dp_E_last, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int ba_hip_marginalize(ba_hip_engine* h, uint32_t nm, const uint32_t* m_ids, uint32_t nl, const uint32_t* l_ids,
                       ba_hip_marginalization_stats* stats) {
  BA_ENTRY_FINAL(h);
  const auto t0 = std::chrono::steady_clock::now();
  if ((nm && !m_ids) || (nl && !l_ids)) return e->fail_msg("marginalize: NULL argument");
  BA_ASK(guard_marginalize(e->held, guard_facts(e), e->st.K != 0));
  const Structure& st = e->st;
  MargPlan pl;
  std::string err;
  if (!marg_plan(e->prob, e->lm_dim, e->pose_dim, st.pose_opt, st.lm_ptr, st.obs_perm, st.R, st.lrow_base, e->dpri, m_ids, nm,
                 l_ids, nl, pl, err)) {
    e->err = err;
    return -1;
  }
  std::vector<uint16_t> lmask(pl.local_pose.size());
  for (size_t i = 0; i < lmask.size(); ++i) lmask[i] = e->mask_host.empty() ? 0 : e->mask_host[pl.local_pose[i]];
  const double tol = e->opt.pivot_rel_tolerance > 0 ? e->opt.pivot_rel_tolerance : 1e-10;
  double dev_ms = 0.0;
  const int rc = marginalize_run(e, pl, lmask, tol, &dev_ms);
  if (rc) {
    e->held.marginalize_failed();
    return rc;
  }
  // x0: the state of the blanket poses at this linearisation
  std::vector<double> state((size_t)st.P * kPoseState);
  BAE_HIP(hipMemcpy(state.data(), e->pose_state[e->cur].p, state.size() * sizeof(double), hipMemcpyDeviceToHost));
  e->marg_ids.assign(pl.local_pose.begin() + pl.nM, pl.local_pose.end());
  e->marg_x0.resize(e->marg_ids.size() * kPoseState);
  for (size_t i = 0; i < e->marg_ids.size(); ++i)
    for (int k = 0; k < kPoseState; ++k) e->marg_x0[i * kPoseState + k] = state[(size_t)e->marg_ids[i] * kPoseState + k];
  e->held.marginalized();
  if (stats) {
    *stats = ba_hip_marginalization_stats();
    stats->blanket_poses = pl.nB;
    stats->absorbed_projection = pl.n_proj; stats->absorbed_unary = pl.n_unary; stats->absorbed_binary = pl.n_binary;
    stats->absorbed_inertial = pl.n_imu; stats->absorbed_priors = pl.n_prior; stats->dropped_projection = pl.n_dropped;
    stats->device_ms = dev_ms;
    stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return 0;
}

int ba_hip_get_marginalization(ba_hip_engine* h, uint32_t* blanket_ids, double* x0_16, double* H, double* b, double* c) {
  BA_ENTRY_HOST(h);
  if (!e->held.marg_valid) return e->fail_msg("ba_hip_get_marginalization: no marginalisation result (ba_hip_marginalize)");
  if (blanket_ids) std::copy(e->marg_ids.begin(), e->marg_ids.end(), blanket_ids);
  if (x0_16) std::copy(e->marg_x0.begin(), e->marg_x0.end(), x0_16);
  if (H) std::copy(e->marg_H.begin(), e->marg_H.end(), H);
  if (b) std::copy(e->marg_b.begin(), e->marg_b.end(), b);
  if (c) *c = e->marg_c;
  return 0;
}

int ba_hip_release_marginalization(ba_hip_engine* h) {
  BA_ENTRY_HOST(h);
  e->held.marginalization_released();
  std::vector<uint32_t>().swap(e->marg_ids);
  std::vector<double>().swap(e->marg_x0);
  std::vector<double>().swap(e->marg_H);
  std::vector<double>().swap(e->marg_b);
  e->marg_c = 0.0;
  return 0;
}

int ba_hip_select_kth(ba_hip_engine* h, uint32_t n, const double* values, uint32_t k, double* out) {
  BA_ENTRY_DEVICE(h);
  DBuf<double> dv;
  BAE_HIP(dv.alloc(std::max<uint32_t>(n, 1)));
  BAE_HIP(e->hist.alloc(2048 + 8));
  if (n) BAE_HIP(hipMemcpy(dv.p, values, (size_t)n * 8, hipMemcpyHostToDevice));
  return select_kth(e, dv.p, n, k, out);
}

}  // extern "C"
