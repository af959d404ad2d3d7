// Internal declarations of the gfx950 engine behind include/ba_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ba_hip.h"
#include "structure.h"
#include "ordering.h"
#include "selinv.h"
#include "marg.h"
#include "pcg.h"
#include "dist_plan.h"
#include "lifecycle.h"
#include "chol_launch.h"
#include "bulk_lists.h"
#include "damping.h"
#include "triang.h"
#include "resect.h"

namespace bae {

// ---- owning device buffer: freed by its destructor (DESIGN.md "ownership") ---------
// bytes held by every DBuf of the process (ba_hip_device_bytes_live)
inline std::atomic<int64_t> g_device_bytes_live{0};
template <typename T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  DBuf(DBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DBuf& operator=(DBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~DBuf() { release(); }
  hipError_t alloc(size_t count) {
    if (count <= n && p) return hipSuccess;
    release();
    if (count == 0) { n = 0; return hipSuccess; }
    hipError_t err = hipMalloc((void**)&p, count * sizeof(T));
    if (err == hipSuccess) { n = count; g_device_bytes_live += (int64_t)bytes(); }
    return err;
  }
  void release() {
    if (p) { (void)hipFree(p); g_device_bytes_live -= (int64_t)bytes(); }
    p = nullptr;
    n = 0;
  }
  size_t bytes() const { return n * sizeof(T); }
};

// bulk_lists.h on the device: all launches of a solve in one buffer of (block row, block column) in absolute
// 128-block coordinates, ~0 for a sentinel; the per-launch slices stay on the host.
struct BulkDeviceLists {
  BulkListsKey key;
  bool built = false;                     // false: grid launches (no pattern, over the budget, BA_HIP_BULK_GRID)
  std::vector<BulkLaunchList> launches;
  DBuf<uint2> blocks;
  uint64_t total_blocks = 0;
  double build_ms = 0.0;                  // host time of the last build and upload
  uint32_t builds = 0;
  const BulkLaunchList* find(uint32_t a_end) const {
    if (!built) return nullptr;
    for (const BulkLaunchList& l : launches)
      if (l.a_end == a_end) return &l;
    return nullptr;
  }
};

// Rigid transform in matrix form as stored on the device: R row-major (9) then t (3).
static const int kRt = 12;
static const int kCamRec = 37;  // camera record: params(4) | T_vs Rt(12) | T_sv Rt(12) | T_vs as t,q (7) | w | model
// Pose state row: t(3) q(4) v(3) b(6)
static const int kPoseState = 16;
// one factor row: 6 doubles (see DESIGN.md "factor rows")
static const int kRow = 6;

// The static structure of the current graph (ba_hip_finalize): the lists of structure.h
using Structure = Lists;

struct Engine {
  int lm_dim = 1, pose_dim = 6, device = 0;
  // Calibration unknowns behind the pose unknowns of the reduced system (ba_hip_set_calibration):
  // 0, or 6 = the decoupled update of T_vs of camera 0 (the reference's DoTvs instantiations).
  int calib_dim = 0;
  // calib_tvs: the six unknowns are T_vs; otherwise (calib_dim == 4 | 5) the parameters of camera 0 — (fx, fy,
  // u0, v0) of a LinearCamera, (fx, fy, u0, v0, w) of a FovCamera (CalibSize; BundleAdjuster.cpp:46-69, parallel_algos.h:114-118)
  bool calib_tvs = false;
  std::vector<double> cam_params_prev;   // params_backup of SolveInternal (:1025-1028): restored by a rollback
  std::vector<double> cam_w_prev;        // ... its fifth entry for a FOV camera
  bool has_fov = false;                  // some camera of the rig is a FovCamera: the FOV kernel instantiations run
  DBuf<double> lm_zref;                  // [L][2] reference pixel of every landmark (LandmarkT::z_ref)
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;   // bulk trailing updates of the factorisation (look-ahead)
  std::vector<hipEvent_t> ev_panel, ev_bulk;
  hipEvent_t ev_imu_start = nullptr, ev_imu_done = nullptr;  // k_imu on stream2 (launch_imu_early)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;           // k_pose_blocks on stream2 (launch_gather_S)
  bool imu_early_pending = false;
  bool own_stream = false;
  std::string err;
  ba_hip_options opt;
  Problem prob;
  Structure st;
  // every "is this still good" flag of what the device holds, and the events that change them (lifecycle.h)
  Held held;
  int cur = 0;  // current state buffer (0/1)
  ba_hip_timers timers;
  ba_hip_allreduce_fn allreduce = nullptr;
  void* allreduce_ctx = nullptr;
  ba_hip_collective_fn coll = nullptr;   // broadcast / reduce-scatter: distributed reduced solve
  void* coll_ctx = nullptr;
  // pose ordering (ba_hip_set_pose_ordering, ordering.h): mode for the next finalize, the caller's permutation
  // (USER), and what the last finalize applied: opt_of_natural[natural opt index] = factorised index (empty:
  // identity), the group graph it was chosen from, its statistics
  int order_mode = kOrderNatural;
  std::vector<uint32_t> order_user;
  std::vector<uint32_t> opt_of_natural;
  std::vector<uint32_t> group_ptr, group_adj;
  ba_hip_ordering_stats order_stats = {};
  bool ordering_refused() const { return allreduce || coll || comm; }
  int rank = 0, nranks = 1;
  // native RCCL communicator (ba_hip_comm_init, comm.hip); comm_force: run the sharded code paths
  // even with one rank (exercises the RCCL calls on a one-GPU box)
  void* comm = nullptr;
  bool comm_force = false;
  bool sharded() const { return allreduce && (nranks > 1 || comm_force); }

  // ---- device: static problem data
  DBuf<double> cam;                 // [C][4 + 12 (T_vs) + 12 (T_sv) + 7 (T_vs as t, q)]
  // With T_vs a parameter the reference reads it in two places: the rig (Jacobian chains) and the
  // per-pose caches of T_sw (PoseT::GetTsw, Types.h:61-70), and a rejected step restores the caches
  // but not the rig (BundleAdjuster.cpp:1060-1068).  `cam` is the rig; cam_eval feeds k_pose_prep
  // (the caches) and differs from it only between a rollback and the next accepted/applied step.
  DBuf<double> cam_eval;
  std::vector<double> tvs_eval, tvs_eval_prev;   // host copies, [C][7]
  const double* cam_eval_ptr() const { return calib_dim ? cam_eval.p : cam.p; }
  DBuf<double> pose_cam;            // [P][4] per-pose intrinsics (Options::use_per_pose_cam_params)
  const double* pose_cam_ptr() const { return prob.pose_cam_params.empty() ? nullptr : pose_cam.p; }
  DBuf<int32_t> pose_opt, lm_opt;
  DBuf<uint16_t> pose_mask;
  // pose_mask holds the masks of the last ba_hip_set_pose_masks.  What reads the Jacobians of the last linearisation
  // after the fact (k_pplever.hip) needs the masks that linearisation ran with: pose_mask itself while
  // mask_version == lin_mask_version, afterwards pose_mask_lin, which ba_hip_set_pose_masks fills before it overwrites
  // pose_mask for the first time since that linearisation.  (Version counters: beside the record of lifecycle.h.)
  DBuf<uint16_t> pose_mask_lin;
  uint64_t mask_version = 0, lin_mask_version = 0;
  const uint16_t* lin_pose_mask() const { return mask_version == lin_mask_version ? pose_mask.p : pose_mask_lin.p; }
  DBuf<uint32_t> lm_ref_pose, lm_ref_cam;
  DBuf<uint32_t> lm_ptr;            // [L+1] CSR over sorted observations
  DBuf<double> obs_z;               // [O][2]
  DBuf<uint32_t> obs_pose, obs_cam, obs_lm, obs_rid;
  DBuf<double> obs_w0;
  DBuf<uint8_t> obs_cond;                // 1 = conditioning residual (ba_hip_set_conditioning_residuals)
  // static lists of structure.h
  DBuf<uint2> wave_rng;                  // [n_chunks] observation ranges of the linearisation waves
  DBuf<uint32_t> tile_ptr;               // [tiles_lower+1]
  DBuf<uint2> tile_ref;                  // (first term, count << 14 | offsets) per block overlapping a tile
  DBuf<uint32_t> tile_order;             // launch order of the tile assembly (build_tile_order)
  DBuf<uint4> tile_desc;                 // per launch entry: (tile, first ref, end ref, row << 16 | column) (k_tile_desc)
  uint32_t n_tile_order = 0;
  uint64_t tile_order_version = ~0ull;
  uint64_t tile_order_plan = ~0ull;      // distributed solve: the launch list holds the owned + sent tiles of the plan with key ..
  int dbg_assemble_variant = 5;          // k_assemble_tiles<VAR> (ba_hip_debug_set key 1)
  int dbg_host_structure = 0;            // 1: build the static lists on the host (structure.h) (key 5)
  int dbg_linearize_variant = 0;         // 0 LDS-staged factor rows, 1 direct stores (key 4)
  int dbg_tile_order = 0;                // 0 row-major tiles, 1 XCD-aware columns (key 2)
  int dbg_imu_wave = -1;                 // k_imu: -1 by count, 0 lanes, 1 wavefront per residual, 2 fused single pass, 4 wavefront per residual and per sample (key 6)
  int dbg_all_tiles = 0;                 // 1: assemble / zero every lower tile, not only the factor's pattern (key 3)
  DBuf<uint2> pair_ent;                  // (rowA, rowB) rank-1 terms of the off-diagonal blocks
  DBuf<uint32_t> pose_ptr, pose_mid;     // [Pact+1], [Pact]
  DBuf<uint32_t> pose_ent;               // 3 x n_pose_entries: (rowA, rowB, scalar index)
  DBuf<uint8_t> nzL;                     // tile pattern of the factor L (nt x nt bytes, lower), see k_chol.hip
  std::vector<uint8_t> nzL_host;         // host copy (flop accounting of the profiled launches)
  uint64_t nzL_version = 0;
  // The non-empty 128-blocks of the bulk updates of cholesky_solve on nzL (bulk_lists.h): rebuilt when `key` (the
  // pattern version and the inputs of the set of launches) moves, as the other version-counted plans.
  BulkDeviceLists bulk_lists;
  std::vector<uint8_t> nzS_host;         // tile pattern of S itself (union over the shards), before fill
  // Distributed solve (dist_solve.hip).  `key`: the dist_plan_key the plan was built for (~0 = none; the plan also
  // remembers nblk, the ranks and the rank).  A new plan rebuilds `tab` (dist_plan.h), so every table below lives and
  // dies with the key; tile_order_plan compares against it.
  struct Dist {
    uint64_t key = ~0ull;
    DistPlan plan;                       // ownership map, per-panel row lists and messages
    DistTables tab;                      // the tables derived from it
    // ... on the device
    DBuf<uint32_t> tiles;                // DistPlan::tiles
    DBuf<uint2> pairs;                   // tab.own.pairs (k_update128<false, true>)
    DBuf<uint32_t> square_rows;          // tab.square_rows
    DBuf<uint32_t> dense_rows;           // tab.dense.rows (reduce-scatter of S)
    DBuf<uint4> send_rects, recv_rects;  // tab.sparse.send / recv (sparse exchange of S)
    // staging
    DBuf<double> msg;                    // square broadcast message
    DBuf<double> usend, urecv;           // urgent point-to-point staging (chain stream)
    DBuf<double> ssend, srecv;           // side point-to-point staging (side stream)
    DBuf<double> back;                   // backward substitution: partial sums of a panel + their reduction
    hipStream_t stream3 = nullptr;       // bulk trailing updates
    hipStream_t stream4 = nullptr;       // side communicator
    void* comm2 = nullptr;               // side communicator (ncclCommSplit of comm)
    std::vector<hipEvent_t> ev;          // 5 events per panel: urgent, packed, side, next, bulk
  } dist;
  // who shares the solve changed (ba_hip_set_allreduce, ba_hip_comm_init, ba_hip_comm_destroy)
  void sharding_changed() { held.sharding_changed(); dist.key = ~0ull; }
  std::string dist_layout_name;
  ba_hip_comm_stats cstats = {};
  DBuf<double> packed;                   // packed lower triangle + rhs row (all-reduce staging)

  // pose-pose residuals (unary | binary | imu slots)
  DBuf<uint8_t> pose_active;
  DBuf<uint32_t> un_pose; DBuf<double> un_t, un_cov_inv, un_scale; DBuf<uint8_t> un_rot;
  DBuf<uint32_t> bin_p1, bin_p2; DBuf<double> bin_t, bin_cov_inv, bin_cov_inv_sqrt, bin_w;
  DBuf<uint8_t> bin_rot;
  DBuf<uint32_t> imu_p1, imu_p2, imu_ptr; DBuf<double> imu_meas, imu_consts, imu_cov_inv;
  // Options::calculate_inertial_covariance_once: per residual 10x10 integration covariance + 10x6
  // bias Jacobian of its first linearisation, and a "done" flag
  bool imu_cov_once = false;
  DBuf<double> imu_frozen;
  DBuf<double> imu_steps;                // [samples][160] step Jacobians of the pre-integration (k_imu_steps)
  DBuf<uint8_t> imu_cov_done;
  uint32_t imu_cov_count = 0;
  DBuf<double> pp_h, pp_g, pp_dz, pp_info, pp_err;
  DBuf<uint32_t> pp_ptr, pp_res_p1, pp_res_p2;
  DBuf<uint4> pp_ent;

  // ---- device: state (double buffered)
  DBuf<double> pose_state[2];            // [P][16]
  DBuf<double> lm_x[2];                  // [L][4]  x_s (lm_dim 1) or x_w (lm_dim 3)
  DBuf<uint8_t> lm_reliable[2];
  DBuf<double> lm_xw;                    // [L][4]  world points (upload / download, lm_dim 1)
  DBuf<double> tsw, tws, twp;            // [P*C][12], [P*C][12], [P][12] for state `cur`
  DBuf<uint32_t> lm_outliers;

  // ---- device: per-iteration
  DBuf<double> obs_e, obs_w;             // error for the median, robust weight
  // err_cache: |r|^2 * original weight per observation at the state held in buffer 0 / 1, left behind by the last
  // EvaluateResiduals at that state (k_residuals mode 1); ba_hip_linearize takes its Huber median from it instead of
  // running the error pass again.  Valid while held.obs_e_valid[buffer]; off with calibration unknowns (the camera
  // moves with the step) and on request (BA_HIP_NO_ERR_CACHE).
  DBuf<double> obs_e_state[2];
  bool err_cache_on() const { return calib_dim == 0 && !err_cache_off; }
  bool err_cache_off = false;
  DBuf<double> obs_jl;                   // [O][2*lm] sqrt(w) * dz_dlm (dogleg J_l * rhs_l)
  DBuf<double> diag_blocks;              // [Pact][36] diagonal blocks of S (k_pose_blocks -> k_write_diag)
  DBuf<double> crow;                     // [n_scalars][6] calibration rows, indexed like `scal`: sqrt(w) dz_dtvs
                                         // (u, v row) of observation a at 2a, 2a+1; E_l = sum w Jl^T Jk of
                                         // landmark l at 2O + l; the last row stays zero
  DBuf<double> border_blocks;            // [Pact][36] S_pk blocks (k_pose_border -> k_write_border)
  DBuf<double> calib_partials;           // block partials of k_calib_reduce
  DBuf<double> frow;                     // [n_rows][6] observation-major factor rows (structure.h)
  DBuf<double> scal;                     // scalars: [2*O] sqrt(w) r, then [L*lm] b_l, then one 0
  DBuf<double> lm_vinv, lm_bl;           // [L][lm*lm], [L][lm]
  DBuf<double> A;                        // [(n+1)][ld] lower storage + rhs row
  DBuf<double> A_keep;                   // copy of A before factorisation (debug option)
  DBuf<double> rhs_p, rhs_sc;            // [n] unreduced / reduced (copy of A's last row)
  DBuf<double> gn_p, gn_l, step_p, step_l;
  DBuf<double> invdiag;                  // inverse diagonal tiles of the Cholesky factor
  DBuf<double> partials;                 // reduction scratch
  DBuf<double> scalars_out;              // small result block (device) + host mirror
  // Deferred scalars: between defer_begin() and defer_flush() the reductions of sum_partials / sum_small
  // leave their results in scalars_out[16 ..) and only note where the host wants them; the flush is ONE
  // device-to-host copy and ONE synchronisation for the whole phase call (a small window pays ~30 us per
  // round trip: four of them made ba_hip_dogleg_terms 140 us).  Off for sharded engines, whose sums go
  // through the all-reduce hook one by one.
  std::vector<hipEvent_t> timer_events;  // pool of the phase timers (engine.hip: EventTimer)
  bool defer_active = false;
  int defer_n = 0;
  double* defer_host[40];
  double dog_h[8];                       // landing place of the dogleg sums (ba_hip_dogleg_terms); [6], [7] reused while held.dog_jrhs_valid
  double eval_h[4];                      // ... of the evaluation sums (ba_hip_eval_residuals)
  DBuf<unsigned long long> hist;         // selection histograms
  DBuf<int32_t> flags;                   // factorisation status block (k_chol.hip: setup_status_block)
  bool square_attr_set = false;          // k_square / k_rowpanel: dynamic LDS limit raised on this engine's device
  DBuf<double> pivot_floor;              // tol * |S_jj| per row (ba_hip_options::pivot_rel_tolerance)
  // marginal covariances (ba_hip_compute_marginals, k_selinv.hip): the selected inverse of the last factor,
  // computed on request only.  sig: one 64x64 slot per lower tile of nzL (selinv.h); the plan is rebuilt when
  // the pattern changes; held.sig_valid: sig belongs to the factor currently in A
  DBuf<double> sig;
  DBuf<uint32_t> sig_slot, sig_col_ptr, sig_col_rows, sig_level_cols, sig_items;
  SelinvPlan sig_plan;
  uint64_t sig_plan_version = ~0ull;
  ba_hip_marginal_stats mstats = {};
  // joint covariances of arbitrary pose sets (ba_hip_get_joint_marginals, k_jointcov.hip): the workspace of the
  // forward substitution Y = L^-1 E and the Gram product, allocated by the first request, reused, freed by
  // ba_hip_release_marginals.  jc_idx: the plan of the last request (jointcov.h)
  DBuf<uint32_t> jc_idx;
  DBuf<double> jc_Y, jc_slots, jc_part, jc_out;
  DBuf<uint32_t> jc_lm;                  // landmark columns (ba_hip_get_joint_state_marginals): ids | tile marks | counts
  ba_hip_joint_marginal_stats jstats = {};
  // solves with the kept factor (ba_hip_factor_solve, k_factorsolve.hip): the plan's tables, one panel per tile
  // row, the partial tiles of a level and the staging of B / X; allocated by the first request, grown on demand,
  // freed by ba_hip_release_marginals
  DBuf<uint32_t> fs_idx;
  DBuf<double> fs_X, fs_slots, fs_B;
  ba_hip_factor_solve_stats fsstats = {};
  // ... and the weakest modes (ba_hip_get_weakest_modes): fs_X then holds three panels of 64 columns; fs_M: the
  // 64 x 64 matrix of an apply and the Ritz values, fs_part: the partial Gram tiles and their sum
  DBuf<double> fs_M, fs_part;
  ba_hip_mode_stats mode_stats = {};
  ba_hip_joint_state_stats jsstats = {};
  ba_hip_leverage_stats lstats = {};     // the last ba_hip_get_projection_leverages (k_lever.hip)
  std::vector<uint32_t> lev_pos;         // its plan (lever.h): sorted position of every residual id, and the block
  uint64_t lev_reads_all = 0;            // reads / landmarks of the all-residuals pass; rebuilt after ba_hip_finalize
  uint32_t lev_lms_all = 0;
  ba_hip_pose_pose_leverage_stats ppl_stats = {};   // the last ba_hip_get_pose_pose_leverages (k_pplever.hip)
  // dense pose priors (ba_hip_set_dense_priors, k_marg.hip): the caller's priors, their device copies (uploaded
  // by ba_hip_finalize), the lower D x D blocks of every prior (dp_blk, prior q from dp_blk_first[q]) and the
  // per-linearisation values: d, J_d, G = J_d^T H J_d, g = J_d^T (b - H d), w = b - H d, E_p
  DensePriors dpri;
  std::vector<uint32_t> dp_blk_first;
  DBuf<uint32_t> dp_ptr, dp_pose;
  DBuf<double> dp_x0, dp_H, dp_b, dp_c;
  DBuf<unsigned long long> dp_hoff;
  DBuf<uint2> dp_blk;
  DBuf<double> dp_d, dp_J, dp_G, dp_g, dp_w, dp_E, dp_E_eval, dp_jr;
  const double* dp_E_last = nullptr;    // E_p of the last linearisation or evaluation (ba_hip_get_prior_errors)
  double prior_err_h = 0.0, prior_jrhs_h = 0.0;
  // marginalisation (ba_hip_marginalize) needs held.lin_valid: the device holds the last linearisation at the
  // current state; pp_err_lin: the pose-pose errors of it; the result (while held.marg_valid) in marg_*
  DBuf<double> pp_err_lin;
  std::vector<uint16_t> mask_host;       // the masks of the last ba_hip_set_pose_masks, by pose id
  std::vector<uint32_t> marg_ids;        // the blanket, by pose id
  std::vector<double> marg_x0, marg_H, marg_b;
  double marg_c = 0.0;

  // iterative reduced solve (ba_hip_set_reduced_solver, k_pcg.hip, pcg.h): the mode of the next ba_hip_solve_gn,
  // its options, the statistics of the last PCG solve (held.pcg_last: the last ba_hip_solve_gn ran PCG, so A still
  // holds S), the plan of nzS_host (rebuilt when the pattern's version changes) and the device work space
  int solver_mode = BA_HIP_SOLVER_DIRECT;
  ba_hip_pcg_options pcg_opt = {};
  ba_hip_pcg_stats pcg_stats = {};
  ba_hip_pcg_coarse_stats pcg_coarse_stats = {};
  uint32_t pcg_coarse_built = 0;  // coarse_aggregate the tables of pcg_plan were built for
  bool pcg_refused() const { return allreduce || coll || comm; }
  PcgPlan pcg_plan;
  std::vector<uint32_t> pcg_blk, pcg_blocks;
  uint64_t pcg_plan_version = ~0ull;
  struct PcgWork {
    DBuf<uint2> tiles, blk, blocks;
    DBuf<uint32_t> row_ptr, col_ptr, col_slot;
    DBuf<uint8_t> nz;
    DBuf<double> rowslot, colslot, minv, x, r, z, p, q, parts;
    DBuf<PcgState> state;
    DBuf<int32_t> status;   // [0] k_pcg_blocks, [1] the coarse factorisation
    // two-level preconditioner (k_pcg_coarse.hip): tables of the plan, C, its factor L, W = L^-1, C^-1, r_c, y_c
    DBuf<uint32_t> cmap, crow_ptr, crow_rows;
    DBuf<double> C, Lc, Wc, Cinv, rc, yc, ryc_part;
    uint32_t coarse_key = 0, coarse_nc = 0, coarse_ncp = 0;   // aggregate the tables were uploaded for; size of the last C
  } pcg;
  // panel PCG (ba_hip_pcg_panel_solve_system, k_pcg_panel.hip, pcg_panel.h): a work space of its own — the tables
  // and vectors of `pcg` belong to the next ba_hip_solve_gn and are not touched — allocated by the first call, grown
  // on demand; the statistics and the per-column record of the last call
  struct PcgPanelWork {
    DBuf<uint32_t> idx;       // chunks | src | blk | blocks | chunk_ptr | rowmap
    DBuf<uint8_t> nz;
    DBuf<double> stage, B, X, P, Z, Q, R, slots, minv, parts, colv;
    DBuf<uint32_t> colu;      // act | run | flags (two copies)
    DBuf<PcgState> state;     // two copies of m_pad states
    DBuf<int32_t> status;
    size_t bytes() const {
      return idx.bytes() + nz.bytes() + stage.bytes() + B.bytes() + X.bytes() + P.bytes() + Z.bytes() + Q.bytes() + R.bytes() +
             slots.bytes() + minv.bytes() + parts.bytes() + colv.bytes() + colu.bytes() + state.bytes() + status.bytes();
    }
  } pcgp;
  ba_hip_pcg_panel_stats pcgp_stats = {};
  std::vector<PcgState> pcgp_cols;

  // Levenberg-Marquardt damping (ba_hip_set_damping, damping.h, k_damp.hip).  lambda_next: what the next
  // ba_hip_linearize takes; lambda_lin: what the linearisation on the device was built with (GuardFacts::damped).
  // The buffers exist only once a linearisation was damped: d_p [n] (engine rows, 0 on masked parameters), d_l
  // [L][lm], schur [Pact][6] the Schur part of the pose diagonals, part / out the sums of k_damp_terms
  // (pred | delta^T D delta | min d | max d), terms_h their host copy while terms_valid.
  struct Damp {
    double lambda_next = 0.0, lambda_lin = 0.0;
    DBuf<double> d_p, d_l, schur, part, out;
    double terms_h[4] = {0, 0, 0, 0};
    bool terms_valid = false;
    double poses_ms = 0.0, terms_ms = 0.0;   // k_damp_poses of the last linearisation, k_damp_terms of the last solve
  } damp;

  // Landmark triangulation (ba_hip_triangulate_landmarks, triang.h, k_triang.hip).  in_solve: between
  // ba_hip_begin_solve and ba_hip_end_solve x_w lags behind x_s (LmSize 1), the call is refused.  The work space exists
  // only once a call was made (ba_hip_release_marginals frees it): mask [L] the selection, early [n_chunks] the waves
  // that left at once, res [L][8] and xw [L][4] the results by landmark id.
  bool in_solve = false;
  struct Tri {
    DBuf<uint8_t> mask, early;
    DBuf<double> res, xw;
    ba_hip_triangulation_stats stats = {};
    void release() { mask.release(); early.release(); res.release(); xw.release(); }
  } tri;

  // Pose refinement with the landmarks held fixed (ba_hip_refine_poses, resect.h, k_resect.hip).  The work space exists
  // only once a call was made (ba_hip_release_marginals frees it).  ptr [P + 1] / idx [O]: the per-pose observation list,
  // built by the first call after a ba_hip_finalize (list_valid; host_ptr its host copy, which sizes the launches);
  // ids / rows [n]: the requests grouped by launch and their result rows; used [O]: the streaming kernel's used flags;
  // res [n][8], t7 [n][7], info [n][36]: the results by request.
  struct Resect {
    DBuf<uint32_t> ptr, idx, ids, rows;
    DBuf<uint8_t> used;
    DBuf<double> res, t7, info;
    std::vector<uint32_t> host_ptr;
    std::vector<uint32_t> host_ids, host_rows;   // the source of the last request's asynchronous uploads: never freed early
    bool list_valid = false;
    ba_hip_pose_refinement_stats stats = {};
    void release() {
      ptr.release(); idx.release(); ids.release(); rows.release(); used.release(); res.release(); t7.release(); info.release();
      host_ptr = std::vector<uint32_t>();
      list_valid = false;
    }
  } resect;

  // optional per-kernel timing (ba_hip_set_profiling)
  bool profiling = false;
  ba_hip_kernel_stats kstats = {};
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_syrk, ev_gather, ev_landmarks, ev_imu, ev_pose;
  void prof_begin(std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, hipStream_t s = nullptr) {
    if (!profiling) return;
    hipEvent_t a, b;
    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    (void)hipEventRecord(a, s ? s : stream);
    v.push_back({a, b});
  }
  void prof_end(std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, hipStream_t s = nullptr) {
    if (!profiling) return;
    (void)hipEventRecord(v.back().second, s ? s : stream);
  }
  void prof_collect();

  // synchronises the streams, destroys the events and the streams the engine created; the members free the rest
  ~Engine();

  int fail(hipError_t e, const char* what);
  int fail_msg(const char* what);
};

// the installed all-reduce (hook or native), with the byte counter of ba_hip_get_comm_stats
inline int shard_allreduce(Engine* e, void* dev_ptr, size_t count, int dtype) {
  e->cstats.allreduce_bytes += 8.0 * (double)count;
  return e->allreduce(e->allreduce_ctx, dev_ptr, count, dtype);
}

#define BAE_HIP(call)                                                    \
  do {                                                                   \
    hipError_t _e = (call);                                              \
    if (_e != hipSuccess) return e->fail(_e, #call);                     \
  } while (0)

// N timing events of one call, destroyed on every exit path.  (Engine::prof_begin keeps its own pairs: those
// are collected later.)
template <int N>
struct Events {
  hipEvent_t ev[N] = {};
  Events() = default;
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  ~Events() {
    for (hipEvent_t v : ev)
      if (v) (void)hipEventDestroy(v);
  }
  hipError_t create() {
    for (hipEvent_t& v : ev) {
      const hipError_t err = hipEventCreate(&v);
      if (err != hipSuccess) return err;
    }
    return hipSuccess;
  }
  hipEvent_t operator[](int i) const { return ev[i]; }
  hipError_t record(int i, hipStream_t s) { return hipEventRecord(ev[i], s); }
  // milliseconds from event a to event b, 0 when the query fails
  double ms(int a, int b) const {
    float t = 0.f;
    return hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? (double)t : 0.0;
  }
};

// `count` host elements into `d` (at least one element is allocated), copied asynchronously on e->stream: the
// source must outlive the stream's next synchronisation.
template <typename T, typename U>
int upload_async(Engine* e, DBuf<T>& d, const U* src, size_t count) {
  static_assert(sizeof(T) % sizeof(U) == 0, "element sizes");
  const size_t n = count * sizeof(U) / sizeof(T);
  BAE_HIP(d.alloc(n ? n : 1));
  if (n) BAE_HIP(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, e->stream));
  return 0;
}

// The index tables of a plan, packed into one device buffer.  add() appends a section and returns its offset in
// words, first padded with zeros to a multiple of `align` words (4 for a section read as uint4, 2 for uint2);
// after an upload into `buf`, at<T>(offset) is the section on the device.
struct IndexPack {
  std::vector<uint32_t> w;
  const uint32_t* d = nullptr;
  template <class It>
  size_t add(It first, It last, size_t align = 1) {
    w.resize((w.size() + align - 1) / align * align, 0);
    const size_t o = w.size();
    w.insert(w.end(), first, last);
    return o;
  }
  size_t add(const std::vector<uint32_t>& v, size_t align = 1) { return add(v.begin(), v.end(), align); }
  size_t size() const { return w.size(); }
  hipError_t upload(const DBuf<uint32_t>& buf) {   // synchronous, into a buffer the caller allocated with size() words
    d = buf.p;
    return w.empty() ? hipSuccess : hipMemcpy(buf.p, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  }
  int upload_async(Engine* e, DBuf<uint32_t>& buf) {   // on e->stream: the pack must outlive its next synchronisation
    const int rc = bae::upload_async(e, buf, w.data(), w.size());
    d = buf.p;
    return rc;
  }
  template <class T = uint32_t>
  const T* at(size_t offset) const { return reinterpret_cast<const T*>(d + offset); }
};

// The factor that the last ba_hip_solve_gn left behind, for the kernels that read it: its tile count, the pivot
// signs D and the L_JJ^-T of the diagonal tiles (both in invdiag).  `who` starts the message when there is none.
inline int kept_factor(Engine* e, const char* who, uint32_t* nt, const double** dsgn, const double** linvT) {
  const uint32_t n = e->st.ld / 64;
  if (!e->invdiag.p || !e->held.nzL_valid || e->nzL_host.size() != (size_t)n * n)
    return e->fail_msg((std::string(who) + ": no factor of the last ba_hip_solve_gn").c_str());
  *nt = n;
  const FactorWork fw(n);
  *dsgn = e->invdiag.p + fw.dsgn;
  *linvT = e->invdiag.p + fw.linvT;
  return 0;
}

// ---- kernel launchers (defined in k_*.hip); all enqueue on e->stream -------------
int launch_pose_prep(Engine* e);                       // T_sw, T_ws, T_wp of the current state
int upload_cameras(Engine* e, bool eval_only);         // camera table(s) from prob.cam_* / tvs_eval
int launch_reset_rays(Engine* e);                      // x_s rays of the current state from the reference pixels
int launch_calib_border(Engine* e);                    // S_pk, S_kk, rhs_k into A / rhs (after k_write_diag)
int launch_calib_dogleg(Engine* e, int gn_available, ba_hip_dogleg_scalars* out);
int launch_begin_solve(Engine* e);                     // x_s from x_w
int launch_end_solve(Engine* e);                       // x_w from x_s
int launch_residual_vectors(Engine* e, double* d_r2);  // z - pi per observation at the current state
int launch_residuals(Engine* e, int mode);             // mode 0: errors for the median; 1: EvaluateResiduals
int launch_landmarks(Engine* e, double c_huber, int use_robust);  // Jacobians, V, W, rows
int launch_gather_S(Engine* e);
int launch_pack_lower(Engine* e, int unpack);
size_t packed_lower_count(uint32_t n_pad);                        // pair gather -> A, rhs row, masks
int launch_backsub(Engine* e);                         // delta_l
int launch_compose_step(Engine* e, double coef_rhs, double coef_gn, double* norms2_host);
int launch_apply_step(Engine* e);                      // state[cur] -> state[1-cur]
int launch_dogleg(Engine* e, int gn_available, double* h7, bool skip_jrhs);
// damping (k_damp.hip), each a no-op unless the linearisation is damped (e->damp.lambda_lin > 0):
int damp_prepare(Engine* e);             // buffers of a damped linearisation, before launch_landmarks
int launch_pose_schur_diag(Engine* e);   // Schur part of the pose diagonals, on stream2 behind k_pose_blocks
int launch_damp_poses(Engine* e);        // d_p, S_jj += lambda d_p: once A holds the complete S
int launch_damp_terms(Engine* e);        // predicted decrease and delta^T D delta of gn_p / gn_l into damp.terms_h
int select_kth(Engine* e, const double* d_values, uint32_t n_local, uint64_t k, double* out);
int sum_partials(Engine* e, uint32_t nparts, uint32_t ncomp, double* host_out, bool cross_shard = true);
void defer_begin(Engine* e);   // k_reduce.hip
int defer_flush(Engine* e);
// The deferred-sum scope of one phase call (Engine::defer_active).  flush(): the ONE copy and synchronisation, where
// the call wants its sums.  A scope that ends without it (an error return) is cancelled: nothing is copied and
// nothing is written through the host pointers the reductions registered.
struct DeferScope {
  Engine* e;
  bool flushed = false;
  explicit DeferScope(Engine* eng) : e(eng) { defer_begin(e); }
  DeferScope(const DeferScope&) = delete;
  DeferScope& operator=(const DeferScope&) = delete;
  int flush() { flushed = true; return defer_flush(e); }
  ~DeferScope() {
    if (flushed) return;
    e->defer_active = false;
    e->defer_n = 0;
  }
};
int launch_imu_early(Engine* e, double c_huber_proj);
int launch_posepose_build(Engine* e, double c_huber_proj, double* h3);
int launch_posepose_eval(Engine* e, double* h3);
int launch_posepose_jrhs(Engine* e, double* out);
// lists: the block lists of the bulk updates for this pattern (ensure_bulk_lists), null = grid launches
int cholesky_solve(Engine* e, double* dA, uint32_t n, uint32_t ld, double* dx, int* status,
                   const uint8_t* nz_tiles, const BulkDeviceLists* lists = nullptr);
// Builds and uploads the lists of a solve of nblk tiles on the host pattern nz_host unless `lists` already holds them
// for (version, nblk, switches); version ~0: a pattern of its own, always rebuilt.
int ensure_bulk_lists(Engine* e, uint32_t nblk, const uint8_t* nz_host, uint64_t version, BulkDeviceLists* lists);
int factor_tile_pattern(Engine* e);
uint32_t choose_kout(uint32_t nblk);
bool dist_solve_enabled(const Engine* e);
int dist_reduce_scatter_S(Engine* e);
int launch_imu_residual_vectors(Engine* e, double* d_r15);
int build_tile_order(Engine* e);
int build_tile_desc(Engine* e);   // k_reduce.hip
int dist_assembly_tiles(Engine* e, std::vector<uint8_t>* need);  // dist_solve.hip
// the static lists built on the device (structure_dev.hip); same contents as structure.h's host builder
int build_lists_device(Engine* e, const std::function<void(const char*)>& stage);
// Pose ordering of ba_hip_finalize (engine.hip): with e->st.pose_opt holding the natural opt ids, builds the
// group graph from `proj_edges` (group pairs that share a landmark, (a << 32 | b)) and the pose-pose residuals,
// chooses the permutation (AUTO) or takes the caller's (USER), and rewrites e->st.pose_opt.
int order_poses(Engine* e, std::vector<uint64_t>* proj_edges, double device_ms);
bool ordering_wants_graph(const Engine* e);
// broadcast of `count` doubles from `root`, ordered into `s`: native RCCL enqueues without a host
// round trip; with a caller-supplied hook the stream is drained first (hook contract)
int dist_broadcast(Engine* e, double* buf, size_t count, int root, hipStream_t s);
// One group of point-to-point transfers, ordered into `s`: `side` selects the side communicator.  Native
// RCCL: ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd; hook: the stream is drained, sends first (they
// do not block), then the receives.
struct DistXfer { double* buf; size_t count; int peer; bool send; };
int dist_exchange(Engine* e, const std::vector<DistXfer>& x, bool side, hipStream_t s);
// in-place SUM over the ranks of `count` doubles, ordered into `s` (chain communicator)
int dist_allreduce_stream(Engine* e, double* buf, size_t count, hipStream_t s);
void comm_release(Engine* e);
int check_solve_residual(Engine* e, const double* dS, const double* dx, const double* db, double* out2);
int cholesky_solve_dist(Engine* e, double* dA, uint32_t ld, double* dx, int* status, const uint8_t* nz);
int trailing_marginals(Engine* e, const double* dA, uint32_t ld, uint32_t first, uint32_t K, double* cov);
// marginal covariances (k_selinv.hip): the selected inverse of the factor in A (no-op while held.sig_valid); blocks
// out of it (rows in engine order: out[q] = Sigma[ra[q] .. + Da, rb[q] .. + Db]); landmark blocks (ids: landmark
// ids, or null for every active landmark by optimisation index); freeing the store
int marginals_compute(Engine* e);
int marginals_gather(Engine* e, uint32_t n, const std::vector<uint32_t>& ra, const std::vector<uint32_t>& rb, int Da,
                     int Db, double* out);
int marginals_landmarks(Engine* e, uint32_t n, const uint32_t* ids, double* out);
void marginals_release(Engine* e);
// leverages of projection residuals from the selected inverse (k_lever.hip): out[q] = the 2 x 2 block of residual
// ids[q] (checked by the caller), or with null ids of every residual in residual-id order (n = st.O)
int leverages_run(Engine* e, uint32_t n, const uint32_t* ids, double* out);
// leverages of unary / binary / inertial residuals from the selected inverse (k_pplever.hip): per requested residual
// of `kind` (ids within the kind, checked by the caller; null: all n of them in id order) the 15 x 15 blocks C and
// Lambda and the leverage tr(C Lambda); any output may be null
int pose_pose_leverages_run(Engine* e, int kind, uint32_t n, const uint32_t* ids, double* cov, double* info, double* lev);
// joint covariance of the rows `sel` of S (engine numbering) and the landmarks `lms` (ids, their columns after
// those of sel) from the factor in A (k_jointcov.hip): out is M x M on the host, M = |sel| + LM |lms|; reads A,
// invdiag and, for landmarks, the rows of the last linearisation
int jointcov_run(Engine* e, const std::vector<uint32_t>& sel, const std::vector<uint32_t>& lms, double* out);
void jointcov_release(Engine* e);
// the substitution of a joint plan whose tables are on the device (k_jointcov.hip), enqueued on `stream`, one level
// after the other: Y <- L^-1 Y (dsgn unused), or with `transposed` and the plan of the mirrored pattern, which holds
// every tile row (panel t = tile t, pos unused), Y <- L^-T D Y
struct JointPlan;
struct SubstTables {
  const uint4 *chunks, *rows;
  const uint32_t *src, *pos;
};
void joint_subst_launch(hipStream_t stream, const JointPlan& p, const SubstTables& t, bool transposed, const double* A,
                        uint32_t ld, const double* linvT, const double* dsgn, double* Y, double* slots);
// B (n x m row-major, the caller's row order) -> a panel of `count` = rows x mp doubles through rowmap (the caller's
// row of every panel row, kJointNone = kPcgNone for a padding row), zeros in padding rows and columns; and back
// (k_factorsolve.hip).  Enqueued on `stream`.
void panel_scatter_launch(hipStream_t stream, const double* B, uint32_t m, const uint32_t* rowmap, uint64_t count,
                          uint32_t mp, double* X);
void panel_gather_launch(hipStream_t stream, const double* X, uint32_t mp, const uint32_t* rowmap, uint64_t count,
                         uint32_t m, double* out);
// X = S^-1 B with a factor on the device (k_factorsolve.hip): the lower storage A (leading dimension ld = 64 nt),
// its tile pattern on the host, the pivot signs and the L_JJ^-T.  B, X: n x m row-major on the host, rows in the
// caller's order; rowmap (64 nt entries): the caller's row of every factorised row, kJointNone for padding rows
struct FactorRef {
  const double* A;
  uint32_t ld, nt;
  const std::vector<uint8_t>* nz;
  const double *dsgn, *linvT;
};
int factor_solve_run(Engine* e, const FactorRef& f, uint32_t n, const uint32_t* rowmap, uint32_t m, const double* B,
                     double* X);
void factor_solve_release(Engine* e);
// the k eigenpairs of smallest magnitude of the factorised S by the block inverse iteration of factorsolve.h on
// device-resident panels: eigenvalues (k), modes (k x n row-major, rows in the caller's order, unit 2-norm)
struct ModeOptions;
int weakest_modes_run(Engine* e, const FactorRef& f, uint32_t n, const uint32_t* rowmap, uint32_t k, const ModeOptions& o,
                      double* eigenvalues, double* modes);
// dense priors and marginalisation (k_marg.hip): upload at finalize; linearise (mode 1: into A, rhs_p, rhs_p_sc) or
// evaluate (mode 0) every prior at the current state, E_p summed into *err_host; the dogleg term; one marginalisation
int priors_upload(Engine* e);
int launch_priors(Engine* e, int mode, double* err_host);
int launch_priors_jrhs(Engine* e, double* out);
// block-Jacobi PCG on the system in dA (k_pcg.hip): uploads `plan` / the row blocks when `upload` is set, solves
// S x = rhs for the first n unknowns of the padded system into dx (ld doubles), fills *stats; *status != 0 on a breakdown
int pcg_solve_device(Engine* e, const double* dA, uint32_t n, uint32_t ld, const double* d_rhs, const PcgPlan& plan,
                     const std::vector<uint8_t>& nz, const std::vector<uint32_t>& blk, const std::vector<uint32_t>& blocks,
                     bool upload, const ba_hip_pcg_options& opt, double* dx, ba_hip_pcg_stats* stats, int* status);
// two-level preconditioner (k_pcg_coarse.hip): C and C^-1 of the plan's coarse space once per solve; the two coarse
// launches of a pass on the residual r
int pcg_coarse_setup_device(Engine* e, const double* dA, uint32_t ld, const PcgPlan& plan);
void pcg_coarse_apply_device(Engine* e, const PcgPlan& plan, const PcgState* st, const double* r);
// panel PCG on the system in dA (k_pcg_panel.hip): X = S^-1 B for the first n unknowns of the padded system, m
// columns.  B, X: n x m row-major on the host, rows in the caller's order; rowmap (ld entries): the caller's row of
// every matrix row, kPcgNone for padding rows.  Fills e->pcgp_stats and e->pcgp_cols, touches no validity flag;
// *status != 0 when some column broke down
int pcg_panel_solve_device(Engine* e, const double* dA, uint32_t n, uint32_t ld, const PcgPlan& plan,
                           const std::vector<uint8_t>& nz, const std::vector<uint32_t>& blk, const std::vector<uint32_t>& blocks,
                           const uint32_t* rowmap, uint32_t m, const double* B, double* X, const ba_hip_pcg_options& opt,
                           int* status);
// triangulation (k_triang.hip): the selection in tri.mask is on the device; fills tri.res / tri.xw for every landmark
int launch_triangulate(Engine* e, const TriOptions& o);
// pose refinement (k_resect.hip): resect.ids / rows hold the requests grouped as cls counts them (no observations, up
// to 256, up to 1 024, more); fills resect.res / t7 / info by request row.  launch_resect_store: t7 over the poses held
int launch_resect(Engine* e, const RsOptions& o, const uint32_t cls[4]);
int launch_resect_store(Engine* e, uint32_t n);
int marginalize_run(Engine* e, const MargPlan& pl, const std::vector<uint16_t>& lmask, double tol, double* dev_ms);

}  // namespace bae
