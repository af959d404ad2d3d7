/*
 * ba_hip.h — C-ABI of the MI355X (gfx950) engine behind ba::BundleAdjuster<>::Solve().
 *
 * The reference (arpg/ba) has no FFI layer: its boundary is the C++ class template
 * ba::BundleAdjuster (/root/reference/include/ba/BundleAdjuster.h:111-753) whose only
 * non-inline member is Solve() (/root/reference/src/BundleAdjuster.cpp:278-705).  This
 * header is the boundary inserted *inside* Solve(): the host class (include/ba/
 * BundleAdjuster.h in this repo) marshals its problem graph into flat SoA arrays once
 * per Solve() and then drives one Gauss-Newton / dogleg iteration as a short sequence of
 * the calls below; only scalars come back per iteration.  Each entry point names the
 * reference code it replaces.
 *
 * Conventions
 *   - plain C, no C++ or torch types; every pointer argument is caller-owned host memory
 *     that is copied during the call unless stated otherwise;
 *   - every function returns int: 0 = ok, <0 = HIP/runtime failure (ba_hip_last_error()
 *     gives text), >0 = numeric status mirroring ba::OptimizationResult
 *     (BundleAdjuster.h:38-46): BA_HIP_FACTORIZATION_ERROR;
 *   - never throws; no global state; one host thread per engine; calls are synchronous
 *     on return (the engine's stream is drained) unless suffixed _async;
 *   - rigid transforms are 7 doubles [tx,ty,tz,qx,qy,qz,qw]; ids are dense uint32 in
 *     insertion order exactly as the reference's Add* calls return them;
 *   - multi-GPU: one engine per device, each holding ALL poses and its shard of
 *     landmarks/projection residuals; the per-iteration sums that cross shards go
 *     through the caller-supplied all-reduce hook (ba_hip_set_allreduce), e.g. RCCL; with
 *     the collectives hook (ba_hip_set_collectives) the reduced solve itself is distributed.
 */
#ifndef BA_HIP_H
#define BA_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BA_HIP_OK 0
#define BA_HIP_FACTORIZATION_ERROR 4 /* ba::FactorizationError, BundleAdjuster.h:44 */
#define BA_HIP_SOLVER_ERROR 5        /* ba::SolverError,        BundleAdjuster.h:45 */

typedef struct ba_hip_engine ba_hip_engine;

/* Options the device phases need (subset of ba::Options, BundleAdjuster.h:72-107). */
typedef struct {
  double projection_outlier_threshold;            /* BundleAdjuster.cpp:184 */
  int32_t use_robust_norm_for_proj_residuals;     /* BundleAdjuster.cpp:1377 */
  int32_t use_robust_norm_for_inertial_residuals; /* BundleAdjuster.cpp:1513 */
  int32_t use_triangular_matrices;                /* only affects debug downloads of S */
  int32_t keep_reduced_system;                    /* keep a copy of S for ba_hip_get_S after the
                                                     in-place factorisation (the reference's
                                                     write_reduced_camera_matrix, BundleAdjuster.cpp:600-627) */
  double gyro_sigma, accel_sigma, gyro_bias_sigma, accel_bias_sigma; /* BundleAdjuster.h:204-218 */
  /* Rank-deficiency guard of the reduced solve (extension; 0 = off = the reference's behaviour).
   * The reference reports FactorizationError only for a pivot that is EXACTLY zero (Eigen's LDLT /
   * SimplicialLDLT info(), BundleAdjuster.cpp:756-759) — on a numerically singular S whether an
   * elimination cancels to exactly zero is rounding-order luck.  With tol > 0 a pivot d_j with
   * |d_j| < tol * |S_jj| (S_jj = the diagonal entry before elimination) raises
   * BA_HIP_FACTORIZATION_ERROR instead of letting an arbitrary step through. */
  double pivot_rel_tolerance;
} ba_hip_options;

/* The four error sums of EvaluateResiduals / BuildProblem (BundleAdjuster.cpp:144-274,
 * 1340-1537; BundleAdjuster.h:593-602). */
typedef struct {
  double proj_error, binary_error, unary_error, inertial_error;
} ba_hip_errors;

/* Scalars of the dogleg step (BundleAdjuster.cpp:858-1017): squared norms and dot
 * products over the pose (p) and landmark (l) parts of rhs (= J^T r, unreduced) and of
 * the Gauss-Newton step, and the steepest-descent denominator ||J rhs||^2. */
typedef struct {
  double rhs_p_sq, rhs_l_sq;   /* :858 numerator */
  double j_rhs_sq;             /* :906-910 denominator */
  double gn_p_sq, gn_l_sq;     /* :971-973 */
  double rhs_gn_p, rhs_gn_l;   /* dot products for a, b of :994-998 */
  /* calibration part (ba_hip_set_calibration; zeros otherwise): |rhs_k|^2 (:859), |delta_k|^2 of
   * the Gauss-Newton step (:972), their dot product (:997).  j_rhs_sq already includes
   * |J_k rhs_k|^2 (:883-886, 910). */
  double rhs_k_sq, gn_k_sq, rhs_gn_k;
} ba_hip_dogleg_scalars;

/* Norms of the step formed by ba_hip_compose_step (summary_.delta_norm is their sum,
 * BundleAdjuster.cpp:26). */
typedef struct {
  double step_p_norm, step_l_norm;
} ba_hip_step_norms;

/* Per-phase device time of the last iteration, milliseconds (HIP events on the engine's
 * stream); names follow the reference's PrintTimer sites (Utils.h:51-62). */
typedef struct {
  double j_evaluation, robust_weights, jtj_schur, solve, back_substitution,
         evaluate_residuals, apply_update;
} ba_hip_timers;

/* ---- lifetime ------------------------------------------------------------------ */
/* lm_dim in {0,1,3}, pose_dim in {6,9,15} (the reference's LmSize / PoseSize template
 * parameters, BundleAdjuster.h:111-134).  stream: a hipStream_t to run on, or NULL for
 * an engine-owned stream.  Fails (<0) when no HIP device is usable: there is no CPU
 * fallback. */
int ba_hip_create(int lm_dim, int pose_dim, int device, void* stream, ba_hip_engine** out);
void ba_hip_destroy(ba_hip_engine* e);
const char* ba_hip_last_error(const ba_hip_engine* e);
/* Bytes of device memory currently held by the engines' own buffers, summed over all engines of the process
 * (work space of calls in flight included); back at its earlier value once an engine is destroyed. */
uint64_t ba_hip_device_bytes_live(void);
int ba_hip_set_options(ba_hip_engine* e, const ba_hip_options* o);
/* The reference's CalibSize / DoTvs template parameters (BundleAdjuster.h:110-134).  do_tvs != 0:
 * the extrinsics T_vs of camera 0 become six more unknowns BEHIND the pose unknowns of the reduced
 * system (kCalibDim = 6, kTvsOffset = 0; BundleAdjuster.cpp:316-322, 493-583): every vector the
 * calls below size with ba_hip_num_pose_params() grows by ba_hip_num_calib_params() trailing
 * entries (rhs, Gauss-Newton delta, step), ba_hip_get_S returns the bordered (n + 6)^2 matrix, and
 * ba_hip_apply_step moves T_vs by exp_decoupled(T_vs, -delta_k) (:72-83) — read it back with
 * ba_hip_get_cameras.  As in the reference a rolled-back step does NOT restore T_vs (:1060-1068).
 * calib_size = 4 (with do_tvs = 0): the pinhole parameters (fx, fy, u0, v0) of camera 0 become four
 * unknowns the same way (kCamParamsInCalib; BundleAdjuster.cpp:46-69, parallel_algos.h:114-118:
 * dz_dcam_params = -dTransfer_dparams(T_sw_m T_ws_r, z_ref, rho)); needs the reference pixel of every
 * landmark (ba_hip_set_landmark_ref_pixels).  ba_hip_apply_step moves the parameters by -delta_k and
 * re-derives every x_s ray from its reference pixel (:57-68); a rollback restores them (:1066, :1147);
 * read them back with ba_hip_get_camera_params.  calib_size = 5: the same for a FovCamera 0
 * (fx, fy, u0, v0, w; ba_hip_set_camera_models) — the reference's SelfCalBundleAdjuster
 * (BundleAdjuster.h:758-759).  calib_size must equal the parameter count of camera 0 (checked by
 * ba_hip_finalize; the reference's fixed-size assignment at parallel_algos.h:115-118).
 * Both at once is refused (the reference's T_vs block wipes the intrinsics columns it shares a
 * j_kpr_ entry with, :1775-1783), as is any other size.  LmSize 1 only (parallel_algos.h:102-131).
 * Structural: call before ba_hip_finalize. */
int ba_hip_set_calibration(ba_hip_engine* e, int calib_size, int do_tvs);
/* LandmarkT::z_ref (BundleAdjuster.h:476-483): the pixel of every landmark in its reference
 * camera, two doubles per landmark id.  Only the intrinsics calibration reads it. */
int ba_hip_set_landmark_ref_pixels(ba_hip_engine* e, uint32_t n, const double* z_ref2);
/* [fx, fy, u0, v0] of every camera as the engine currently holds them; n = the camera count of
 * ba_hip_set_cameras (a mismatch is an error, nothing is written) */
int ba_hip_get_camera_params(ba_hip_engine* e, uint32_t n, double* params4);

/* ---- problem upload (replaces the AoS graph of Types.h:41-321) -------------------- */
/* calibu::Rig cameras: pinhole params [fx,fy,u0,v0] and T_vs (BundleAdjuster.h:259-263) */
int ba_hip_set_cameras(ba_hip_engine* e, uint32_t n, const double* params4, const double* t_vs7);
/* Camera model of every camera of ba_hip_set_cameras (call after it; it resets them to 0):
 * model 0 = calibu::LinearCamera (pinhole), 1 = calibu::FovCamera with distortion parameter w[c]
 * (pix = K (f(r) p), p = P.xy / P.z, f(r) = atan(2 r tan(w/2)) / (r w) — Devernay & Faugeras 2001; Calibu is
 * not in the reference tree, see oracle/outils.h).  w is read for model 1 only. */
int ba_hip_set_camera_models(ba_hip_engine* e, uint32_t n, const int32_t* model, const double* w);
/* w of every camera (0 for a LinearCamera) as the engine currently holds it; n as above */
int ba_hip_get_camera_fov(ba_hip_engine* e, uint32_t n, double* w);
/* Options::use_per_pose_cam_params (BundleAdjuster.h:96; parallel_algos.h:54-57,
 * BundleAdjuster.cpp:162-176): every projection residual is evaluated with the pinhole
 * intrinsics [fx,fy,u0,v0] of its MEASUREMENT pose (PoseT::cam_params, Types.h:46) instead of the
 * rig camera's.  n = number of poses (checked at ba_hip_begin_solve), n = 0 switches back to the
 * rig intrinsics.  May be called at any time before ba_hip_linearize; not part of the structure. */
int ba_hip_set_pose_cam_params(ba_hip_engine* e, uint32_t n, const double* params4);
/* poses_ (BundleAdjuster.h:292-323); v_w/b may be NULL (zeros) */
int ba_hip_set_poses(ba_hip_engine* e, uint32_t n, const double* t_wp7, const double* v_w3,
                     const double* b6, const uint8_t* is_active);
/* landmarks_ (BundleAdjuster.h:326-367): homogeneous world point, reference pose/camera */
int ba_hip_set_landmarks(ba_hip_engine* e, uint32_t n, const double* x_w4,
                         const uint32_t* ref_pose_id, const uint32_t* ref_cam_id,
                         const uint8_t* is_active);
/* ACCEPTED projection residuals in residual-id order (BundleAdjuster.h:459-513) */
int ba_hip_set_projection_residuals(ba_hip_engine* e, uint32_t n, const double* z2,
                                    const uint32_t* meas_pose_id, const uint32_t* landmark_id,
                                    const uint32_t* cam_id, const double* weight);
/* Projection residuals that are "conditioning" (reference pose inactive, measuring pose active,
 * BundleAdjuster.h:503-510): ids into the list above.  Only SolutionSummary::cond_proj_error uses
 * them; ba_hip_get_conditioning_error returns the sum of |residual|^2 over them at the current state
 * (BundleAdjuster.cpp:692-703), formed on the device. */
int ba_hip_set_conditioning_residuals(ba_hip_engine* e, uint32_t n, const uint32_t* residual_id);
int ba_hip_get_conditioning_error(ba_hip_engine* e, double* proj_sq_sum);
/* unary_residuals_ (BundleAdjuster.h:377-407): prior pose and cov^-1 (6x6 row-major) */
int ba_hip_set_unary_residuals(ba_hip_engine* e, uint32_t n, const uint32_t* pose_id,
                               const double* t_wp7, const double* cov_inv36,
                               const uint8_t* use_rotation);
/* binary_residuals_ (BundleAdjuster.h:425-456): cov^-1 and its square root as computed
 * at Add time, weight */
int ba_hip_set_binary_residuals(ba_hip_engine* e, uint32_t n, const uint32_t* pose1_id,
                                const uint32_t* pose2_id, const double* t_12_7,
                                const double* cov_inv36, const double* cov_inv_sqrt36,
                                const double* weight, const uint8_t* use_rotation);
/* inertial_residuals_ (BundleAdjuster.h:516-546): CSR over the sample table,
 * samples are rows [wx,wy,wz,ax,ay,az,time] (Types.h:222-244) */
int ba_hip_set_imu_residuals(ba_hip_engine* e, uint32_t n, const uint32_t* pose1_id,
                             const uint32_t* pose2_id, const uint32_t* meas_ptr /* n+1 */,
                             const double* meas7, const double* weight);
/* ImuResidualT::IntegrateResidual without Jacobians (Types.h:662-738): RK4 integration of `nmeas`
 * IMU samples [wx,wy,wz,ax,ay,az,time] from the state (t_wp7, v_w3) with biases bg3 / ba3 and
 * gravity g3 — host code, the same source as the device kernels (no engine, no GPU needed).
 * states10 receives max(nmeas, 1) rows [t(3) q(4) v(3)]: the start state, then the state at every
 * later sample (the reference's `poses` vector).  Returns 0, or -1 on a NULL argument. */
int ba_hip_integrate_imu(const double t_wp7[7], const double v_w3[3], const double bg3[3], const double ba3[3],
                         const double g3[3], const double* meas7, uint32_t nmeas, double* states10);
/* The same with the Jacobian outputs of the reference's signature (Types.h:662-738), all optional:
 * dpose_db60 (10 x 6, row-major: state [t q v] over the gyro / accelerometer biases), dpose_dpose100
 * (10 x 10, over the start state) and the covariance c_res100 (10 x 10, in/out: C <- F C F^T + G R G^T
 * per step, r6 = diagonal of R).  As in the reference they are formed only when one of the two
 * Jacobians is asked for and r6 is not NULL. */
int ba_hip_integrate_imu_jacobians(const double t_wp7[7], const double v_w3[3], const double bg3[3],
                                   const double ba3[3], const double g3[3], const double* meas7, uint32_t nmeas,
                                   const double r6[6], double* states10, double* dpose_db60,
                                   double* dpose_dpose100, double* c_res100);
/* ImuResidualT::GetPoseDerivative (Types.h:376-416): k9 = [v; R (w + b_g); R (a + b_a) - g] of the
 * state10 = [t(3) q(4) v(3)] with the two samples interpolated at z_start.time + dt; dk_db54 (9 x 6)
 * and dk_dx90 (9 x 10) may be NULL.  ImuResidualT::IntegratePose (Types.h:324-373): out10 = the state
 * advanced by k9 * dt (q <- exp(k_w dt) q, not renormalised); dy_dk90 (10 x 9) and the quaternion
 * block dy_dy16 (4 x 4) may be NULL.  Host code, no GPU. */
int ba_hip_imu_pose_derivative(const double state10[10], const double g3[3], const double z_start7[7],
                               const double z_end7[7], const double bg3[3], const double ba3[3], double dt,
                               double k9[9], double* dk_db54, double* dk_dx90);
int ba_hip_imu_integrate_pose(const double state10[10], const double k9[9], double dt, double out10[10],
                              double* dy_dk90, double* dy_dy16);
/* The Lie-group / quaternion helpers of the reference's include/ba/Utils.h, host code shared with the kernels
 * (include/ba/Utils.h wraps this entry with the reference's names).  Transforms travel as [t(3) q(4)],
 * quaternions as x,y,z,w; results are row-major.  op: 1 dlog_dq(q) 3x4 | 2 dq_exp_dw(w) 4x3 | 3 dq1q2_dq1(q2) 4x4 |
 * 4 dq1q2_dq2(q1) 4x4 | 5 dqx_dq(q, x3) 3x4 | 6 dqx_dx(q) 3x3 | 7 log_decoupled(a, b) 6 | 8 exp_decoupled(a, x6) 7 |
 * 9 dlog_decoupled_dx(a, b) 6x6 | 10 dLog_decoupled_dt1(t1, t2) 6x7 | 11 dlog_decoupled_dt2(t1, t2) 6x7 |
 * 12 dexp_decoupled_dx(t) 7x6 | 13 dinv_exp_decoupled_dx(t) 7x6 | 14 dt_x_dt(t, x4) 4x7 | 15 dt1_t2_dt1(t1, t2) 7x7 |
 * 16 dt1_t2_dt2(t1) 7x7 | 17 MultHomogeneous(t, x4) 4.  Returns the number of doubles written, -1 on a bad call. */
int ba_hip_lie(int op, const double* a, const double* b, double* out);
/* ImuCalibrationT::r and r_b (Types.h:112-159): diagonal of the IMU measurement noise (gyro x3,
 * accelerometer x3) and of the bias random walk, as parallel_algos.h:204,288 read them from imu_.
 * NULL pointers: derive both from the sigmas of ba_hip_options (what Init() does,
 * BundleAdjuster.h:204-218).  Like the gravity vector it is not part of the structure: it takes
 * effect at the next ba_hip_begin_solve, no ba_hip_finalize needed. */
int ba_hip_set_imu_noise(ba_hip_engine* e, const double r6[6], const double rb6[6]);
/* Options::calculate_inertial_covariance_once (BundleAdjuster.h:106, parallel_algos.h:189-205):
 * the integration covariance and the bias Jacobian of an inertial residual are computed in its
 * first linearisation and reused afterwards (they survive later ba_hip_set_imu_residuals calls
 * as long as the residual list only grows).  reset != 0 forgets the stored ones (Init()). */
int ba_hip_set_inertial_covariance_once(ba_hip_engine* e, int on, int reset);
int ba_hip_set_gravity(ba_hip_engine* e, const double g3[3]); /* BundleAdjuster.h:243-252 */
/* Build the device-side structure: observation list sorted by landmark (CSR),
 * pose-landmark incidences, per-pose-pair gather lists for the reduced matrix. */
int ba_hip_finalize(ba_hip_engine* e);

/* ---- one Solve() ------------------------------------------------------------------ */
/* BundleAdjuster.cpp:288-296: x_s = T_sw(ref) x_w, normalised (lm_dim == 1).  May be called
 * again on a finalized engine whose graph did not change (the reference's "Solve may be called
 * repeatedly", BundleAdjuster.h:549-551): the state, Huber-compounded unary weights, reliability
 * flags and frozen inertial covariances the previous Solve() left on the device are kept. */
int ba_hip_begin_solve(ba_hip_engine* e);
/* BundleAdjuster.cpp:1237-1330 decides the masks on the host; bit i of masks[p] set =
 * parameter i of pose p is regularised (Jacobian column zeroed, S(idx,idx) = 1e6,
 * BundleAdjuster.cpp:587-598,1622-1629). */
int ba_hip_set_pose_masks(ba_hip_engine* e, uint32_t n, const uint16_t* masks);
/* BuildProblem + J^T J + Schur complement (BundleAdjuster.cpp:1166-1803, 327-598):
 * leaves S, rhs_p_sc, rhs_p, rhs_l, V^-1, W on the device; returns the error sums
 * BuildProblem computes (proj_error_ etc.). */
int ba_hip_linearize(ba_hip_engine* e, ba_hip_errors* out);
/* CalculateGn + GetLandmarkDelta (BundleAdjuster.cpp:748-833, 709-744): dense Cholesky
 * of S, delta_p, then delta_l = V^-1 (rhs_l - W^T delta_p). */
int ba_hip_solve_gn(ba_hip_engine* e);
/* BundleAdjuster.cpp:858-925 + the norms/dots of :971-1004 */
int ba_hip_dogleg_terms(ba_hip_engine* e, int gn_available, ba_hip_dogleg_scalars* out);

/* ---- Levenberg-Marquardt damping (ba_amd/csrc/damping.h) ----------------------------
 * With lambda > 0 the next ba_hip_linearize builds, and ba_hip_solve_gn solves, (H + lambda diag(d)) delta = g
 * instead of H delta = g: H = J^T Lambda J the full normal matrix, d_j = min(max(H_jj, 1e-6), 1e32) for every free
 * parameter (masked pose parameters keep their 1e6 and get no damping).  Inside the landmark elimination:
 * V + lambda diag(d_l) is inverted (d_l from diag V after the 1e-6 guard), so the factor rows, V^-1, the Schur part
 * of S and of the right-hand side and the back-substitution are those of the damped system; the pose diagonal of H,
 * recovered as S_jj minus its Schur part, is clamped into d_p and lambda d_p is added to S_jj.
 * lambda = 0 (the default) is the undamped engine: no damping kernel runs, no damping buffer is allocated, and the
 * results are bitwise those of an engine that never saw the call.  lambda > 0 is refused with calibration unknowns
 * (ba_hip_set_calibration) and on an engine that is sharded, hooked or runs the distributed solve.
 * While the linearisation the device holds is damped, ba_hip_dogleg_terms and every reader of the kept factor, of the
 * factor rows or of S for covariances, leverages, modes, panel solves or marginalisation priors refuses: linearise
 * and solve once with damping 0.  ba_hip_get_S and ba_hip_check_solve serve the damped S. */
int ba_hip_set_damping(ba_hip_engine* e, double lambda);   /* >= 0; 0 = off (default); used from the next ba_hip_linearize */
typedef struct {
  double lambda;               /* of the linearisation the device holds */
  /* of the last ba_hip_solve_gn, in the units of ba_hip_errors: E(0) - E_model(delta) = delta^T (lambda D delta + g),
   * and delta^T D delta.  The gain ratio of a step is (E_before - E_after) / predicted_decrease. */
  double predicted_decrease, step_scaled_sq;
  double diag_min, diag_max;   /* over d_p and d_l of the free parameters, after the clamp */
  double device_ms;            /* k_damp_poses of the linearisation + k_damp_terms of the solve */
} ba_hip_damping_terms;
/* zeros (lambda = 0) for an undamped linearisation; needs a finished ba_hip_solve_gn for a damped one */
int ba_hip_get_damping_terms(ba_hip_engine* e, ba_hip_damping_terms* out);
/* test / report access: d_p (ba_hip_num_pose_params, the caller's row order, 0 on masked parameters) and d_l
 * (ba_hip_num_lm_params, by landmark optimisation index) of the damped linearisation; either may be NULL */
int ba_hip_get_damping_diagonal(ba_hip_engine* e, double* d_p, double* d_l);
/* The control rule of the damped step (Nielsen), on the host; the engine's state is not touched: with the gain ratio
 * rho = (E_before - E_after) / predicted_decrease of a step, accepted (returns 1) when rho > 0: lambda <- lambda
 * max(1/3, 1 - (2 rho - 1)^3), nu <- 2; otherwise (returns 0; a NaN ratio included) lambda <- lambda nu, nu <- 2 nu.
 * lambda is kept in [1e-12, 1e12].  nu starts at 2.  Returns -1 for a NULL argument. */
int ba_hip_damping_update(ba_hip_engine* e, double* lambda, double* nu, double rho);
/* step = coef_rhs * (rhs_p_, rhs_l_) + coef_gn * delta_gn  (BundleAdjuster.cpp:923-925,
 * 947-950, 985, 1015-1017, 1108-1110) */
int ba_hip_compose_step(ba_hip_engine* e, double coef_rhs, double coef_gn, ba_hip_step_norms* out);
/* ApplyUpdate (BundleAdjuster.cpp:21-140) into the alternate state buffer; the previous
 * state is kept as the rollback snapshot (replaces the deep copies of :1022-1028). */
int ba_hip_apply_step(ba_hip_engine* e);
/* restore the snapshot (BundleAdjuster.cpp:1060-1068, 1139-1149) */
int ba_hip_rollback(ba_hip_engine* e);
/* EvaluateResiduals (BundleAdjuster.cpp:144-274) at the current state */
int ba_hip_eval_residuals(ba_hip_engine* e, ba_hip_errors* out);
/* BundleAdjuster.cpp:672-678: x_w = T_ws(ref) x_s (lm_dim == 1) */
int ba_hip_end_solve(ba_hip_engine* e);

/* ---- results / debug taps ----------------------------------------------------------- */
int ba_hip_get_poses(ba_hip_engine* e, double* t_wp7, double* v_w3, double* b6);
int ba_hip_get_landmarks(ba_hip_engine* e, double* x_w4);
int ba_hip_get_landmark_flags(ba_hip_engine* e, uint8_t* is_reliable, uint32_t* num_outliers);
uint32_t ba_hip_num_pose_params(const ba_hip_engine* e);   /* PoseSize * active poses */
uint32_t ba_hip_num_calib_params(const ba_hip_engine* e);  /* 0, or 6 with ba_hip_set_calibration(.., do_tvs) */
/* Options::calculate_calibration_marginals (BundleAdjuster.cpp:771-784): the K x K block of S^-1
 * that belongs to the calibration unknowns (row-major), from the factor left by the last
 * ba_hip_solve_gn — no extra solves.  Replicated / single-shard solve only. */
int ba_hip_get_calibration_marginals(ba_hip_engine* e, double* cov_kxk);
/* T_vs of every camera (7 doubles each) as the engine currently holds them: the values of
 * ba_hip_set_cameras, moved by the calibration steps applied since. */
int ba_hip_get_cameras(ba_hip_engine* e, uint32_t n, double* t_vs7);  /* n = camera count, checked */
uint32_t ba_hip_num_lm_params(const ba_hip_engine* e);
/* s_ as the reference leaves it (BundleAdjuster.cpp:473-477,587-598): dense n x n
 * row-major (n = pose + calibration unknowns); block (i,j) kept only for i <= j when
 * use_triangular_matrices (the calibration border counts as the last block: S_pk is kept, S_kp not,
 * :513-518).  The vectors of get_rhs / get_delta_gn / get_step sized by the pose unknowns carry the
 * calibration entries behind them.  After a direct ba_hip_solve_gn S was factorised in place and is read from the
 * copy of keep_reduced_system; after a PCG solve (ba_hip_set_reduced_solver) S is intact and no copy is needed. */
int ba_hip_get_S(ba_hip_engine* e, double* s_nxn);
int ba_hip_get_rhs(ba_hip_engine* e, double* rhs_p_sc, double* rhs_p, double* rhs_l);
int ba_hip_get_delta_gn(ba_hip_engine* e, double* delta_p, double* delta_l);
int ba_hip_get_step(ba_hip_engine* e, double* delta_p, double* delta_l);
int ba_hip_get_proj_weights(ba_hip_engine* e, double* weight); /* per residual id */
/* residual vectors z - pi (2 doubles per residual id) at the current state, i.e. what
 * ProjectionResidual::residual holds after a Solve() (BundleAdjuster.cpp:155-181) */
int ba_hip_get_proj_residuals(ba_hip_engine* e, double* residual2);
/* The weighted Jacobian blocks and residuals of the last ba_hip_linearize as the reference stores
 * them in j_pr_, j_l_ and r_pr_ (BundleAdjuster.cpp:1636-1642, 1795-1796, 1384-1385): per residual id
 * sqrt(w) dz_dx_meas (2x6), sqrt(w) dz_dx_ref (2x6, LmSize 1), sqrt(w) dz_dlm (2xLm) and
 * sqrt(w) r (2), masked columns zeroed.  Read back from the factor rows — the device never holds a
 * Jacobian MATRIX; the host class writes the reference's j_pr.txt / j_l.txt / r_pr.txt from this
 * (write_reduced_camera_matrix, BundleAdjuster.cpp:608-616).  Any pointer may be NULL. */
int ba_hip_get_proj_jacobians(ba_hip_engine* e, double* j_meas12, double* j_ref12, double* j_lm, double* r2);
/* Calibration instantiations: sqrt(w) dz_dtvs (2x6) per residual id, what the reference stores in
 * j_kpr_ (BundleAdjuster.cpp:1769-1783) and writes to j_kpr.txt (:619-622). */
int ba_hip_get_calib_jacobians(ba_hip_engine* e, double* j_k12);
int ba_hip_get_timers(ba_hip_engine* e, ba_hip_timers* t);
/* Test tap for systems too large to download (S is 28.8 GB at BASELINE.json configs[3]): forms
 * || S delta_gn - rhs_p_sc || and || rhs_p_sc || ON THE DEVICE from the copy of S kept before the
 * in-place factorisation (needs ba_hip_options.keep_reduced_system) and the Gauss-Newton pose
 * step of the last ba_hip_solve_gn — i.e. checks what CalculateGn promises,
 * S delta = rhs (BundleAdjuster.cpp:748-833).  Single shard only.  After a PCG solve (ba_hip_set_reduced_solver)
 * it runs on S itself, without keep_reduced_system. */
int ba_hip_check_solve(ba_hip_engine* e, double* residual_norm, double* rhs_norm);
/* Residual vectors of the inertial residuals at the current state (ImuResidualT::residual after
 * EvaluateResiduals, BundleAdjuster.cpp:225-256): 15 doubles per residual in residual-id order,
 * the first PoseSize of them used (9: translation, rotation, velocity; 15: + biases). */
int ba_hip_get_imu_residuals(ba_hip_engine* e, double* residual15);
/* Mahalanobis distance of every inertial residual at the last evaluation (ImuResidualT::
 * mahalanobis_distance, BundleAdjuster.cpp:252-254), residual-id order; summed over the
 * conditioning residuals by SolutionSummary::cond_inertial_error (:680-690). */
int ba_hip_get_imu_errors(ba_hip_engine* e, double* mahalanobis);
/* cumulative Huber scale of every unary residual's cov^-1 (the reference multiplies
 * cov_inv in place every BuildProblem, BundleAdjuster.cpp:1469) */
int ba_hip_get_unary_scales(ba_hip_engine* e, double* scale);
/* restores them (n = the unary residual count): a caller that relinearises outside a Solve() (the host
 * class's Marginalize) puts back what the extra BuildProblem compounded */
int ba_hip_set_unary_scales(ba_hip_engine* e, uint32_t n, const double* scale);

/* Per-kernel device time, accumulated since ba_hip_set_profiling(e, 1): HIP events on
 * the engine's stream around every launch of the three hot kernels (used by bench.py's
 * roofline; costs two events per launch, so it is off by default). */
typedef struct {
  uint32_t syrk_launches, gather_launches /* k_assemble_tiles */, landmarks_launches /* k_linearize */, imu_launches;
  double syrk_ms, gather_ms, landmarks_ms;
  double syrk_flops;       /* algorithmic flops of those k_syrk launches */
  double imu_ms;           /* k_imu, the BuildProblem launch (parallel_algos.h:178-358) */
  double pose_blocks_ms;   /* k_pose_blocks: diagonal blocks + right-hand sides */
  uint32_t pose_blocks_launches, reserved;
} ba_hip_kernel_stats;
/* Sizes of the static structure ba_hip_finalize built (for byte accounting in benchmarks). */
typedef struct {
  uint64_t poses_active, landmarks_active, observations;
  uint64_t incidences;        /* (active pose, active landmark) pairs */
  uint64_t factor_rows;       /* 48-byte rows written by the linearisation kernel per iteration */
  uint64_t pair_blocks;       /* off-diagonal pose-pair blocks of S with at least one term */
  uint64_t pair_entries;      /* rank-1 terms summed into those blocks */
  uint64_t tiles_lower;       /* 64x64 tiles of the lower triangle incl. diagonal */
  uint64_t tiles_S, tiles_L;  /* of those: structurally nonzero in S / in its factor (after fill) */
  uint64_t tile_refs;         /* (tile, block) references of the tile assembly (straddling blocks count twice) */
  uint64_t pose_entries;      /* terms of the diagonal blocks / right-hand sides (12 bytes each) */
  uint64_t linearize_waves;   /* wavefronts of the linearisation kernel */
  uint64_t factor_tile_products; /* 64x64x64 tile products of the tile-sparse LDL^T on the factor's pattern (trailing
                                    updates + substitutions; x 2 * 64^3 flop each): the flops of one reduced solve */
} ba_hip_structure_stats;
int ba_hip_get_structure_stats(ba_hip_engine* e, ba_hip_structure_stats* out);
/* Experiment knobs for scratch/ micro-benchmarks (kernel variants with identical results): key 1 =
 * variant of the tile assembly kernel (0, 1, 2, 6; 5 is what runs; any other value is refused),
 * key 2 = launch order of its tiles (0 row-major, 1 XCD-aware columns), key 3 = 1: write every lower tile instead of the factor's pattern only,
 * key 4 = linearisation variant (0 LDS-staged rows, 1 direct stores), key 5 = 1: build the static
 * lists on the host (structure.h) instead of on the device at the next ba_hip_finalize, key 6 = variant
 * of the inertial linearisation (-1 chosen by residual count, 0 one lane per sample / per residual, 1 a
 * wavefront per residual over the lane-per-sample step pass, 2 the single-pass form with the step Jacobians
 * inside, 4 a wavefront per residual AND per sample). */
int ba_hip_debug_set(ba_hip_engine* e, int key, int value);
int ba_hip_set_profiling(ba_hip_engine* e, int enable);
int ba_hip_get_kernel_stats(ba_hip_engine* e, ba_hip_kernel_stats* out);

/* ---- raw device access for drivers that own streams/collectives ---------------------- */
/* Device pointer + element count of the buffers whose cross-shard SUM defines the
 * iteration: 0 = S (lower storage incl. rhs row), 1 = scalar block. */
int ba_hip_device_buffer(ba_hip_engine* e, int which, void** dev_ptr, size_t* num_doubles);
/* All-reduce hook: called on the engine's host thread, after the engine has drained its
 * stream, for every buffer that must be summed over shards (doubles or uint64 counts).
 * dtype: 0 = f64, 1 = u64.  Must return 0 on success.  NULL = single shard. */
typedef int (*ba_hip_allreduce_fn)(void* ctx, void* dev_ptr, size_t count, int dtype);
int ba_hip_set_allreduce(ba_hip_engine* e, ba_hip_allreduce_fn fn, void* ctx, int rank, int nranks);
/* Cross-shard SUM of `count` host values (dtype 0 = f64, 1 = u64) through the installed all-reduce
 * (hook or native communicator); a no-op on a single shard.  Used by the host class for the few
 * graph statistics the gauge masks depend on (BundleAdjuster.cpp:1237-1330): per-pose residual
 * counts must be GLOBAL counts when the residuals are sharded. */
int ba_hip_allreduce_host(ba_hip_engine* e, void* host, size_t count, int dtype);
/* Collectives hook (optional, on top of the all-reduce hook): with it the dense reduced solve
 * is DISTRIBUTED over the shards instead of replicated:
 * S is cut into blocks of G x G 64-tiles (G = 4 / 8 / 16 by system size) owned by the ranks through a small class
 * table (ba_amd/csrc/dist_plan.h: "tri" / "grid" / "col" / "row" layouts); the partial S of every shard reaches the
 * block owners point to point (only the rectangles the shard's own pattern touches), the owner of a diagonal block
 * factorises the panel's square and broadcasts it, the block rows under it travel point to point to the ranks that
 * multiply them, and each rank applies the trailing updates to the tiles it owns.
 *   op 1 = broadcast `count` doubles at dev_ptr from rank `root`;
 *   op 2 = reduce-scatter (sum), in place: dev_ptr holds nranks chunks of `count` doubles, on
 *          return chunk `rank` (at dev_ptr + rank * count) holds the sum over ranks of that chunk
 *          (BA_HIP_DENSE_SCATTER=1 and single-rank communicators only);
 * Same calling conventions as the all-reduce hook.  NULL = replicated solve. */
typedef int (*ba_hip_collective_fn)(void* ctx, int op, void* dev_ptr, size_t count, int root);
/* (ops 3 / 4 / 5 of the hook, used by the distributed solve since round 3: op 3 = send `count` doubles at
 * dev_ptr to rank `root`, must not block on the receiver (copy or defer); op 4 = receive `count` doubles from rank
 * `root`; op 5 (dev_ptr NULL) = end of one exchange: every send handed over since the last op 5 has been started.
 * The engine issues all sends of an exchange, then all receives, then op 5.) */
int ba_hip_set_collectives(ba_hip_engine* e, ba_hip_collective_fn fn, void* ctx);
/* Native communicator: the engine loads librccl itself (one process per GPU, RCCL over xGMI) and
 * runs every cross-shard sum and the collectives of the distributed reduced solve on an
 * engine-owned ncclComm — a C++ user of ba::BundleAdjuster needs no torch and no hooks.
 *   ba_hip_comm_unique_id  rank 0 creates the 128-byte id and hands it to the other ranks out of band
 *   ba_hip_comm_init       collective over all ranks (ncclCommInitRank on the engine's device);
 *                          installs the native all-reduce + collectives (replacing any hook) and sets
 *                          rank / nranks.  nranks == 1 is allowed and still drives the sharded code
 *                          paths through RCCL (test on a one-GPU box)
 *   ba_hip_comm_destroy    back to a single unsharded engine
 * With it the per-panel broadcast of the distributed solve is enqueued in stream order (no host
 * round trip per panel). */
int ba_hip_comm_unique_id(void* id128);
int ba_hip_comm_init(ba_hip_engine* e, const void* id128, int rank, int nranks);
int ba_hip_comm_destroy(ba_hip_engine* e);
/* Bytes this rank moved through the communicator(s) since the last reset: the chain stream carries what
 * the next panel waits for (factorised squares, the block row under them, the backward substitution's
 * partial sums), the side stream the rest of every panel (consumed by the bulk trailing updates). */
typedef struct {
  double chain_bytes_sent, chain_bytes_recv;   /* square broadcasts (root: sent, others: received) + urgent rows */
  double side_bytes_sent, side_bytes_recv;     /* the remaining rows of every panel, point to point */
  double reduce_scatter_bytes;                 /* partial S onto the tile owners (send buffer size per call) */
  double allreduce_bytes;                      /* every all-reduced buffer (rhs, scalars, histograms, patterns) */
  uint64_t chain_messages, side_messages, factorisations;
} ba_hip_comm_stats;
int ba_hip_get_comm_stats(ba_hip_engine* e, ba_hip_comm_stats* out);
int ba_hip_reset_comm_stats(ba_hip_engine* e);
/* Byte accounting of the distributed solve's message plan WITHOUT a device (pure host): nz_lower is the
 * nblk x nblk row-major byte pattern of the factor's 64x64 tiles (NULL = dense), layout one of "auto",
 * "tri", "grid", "col", "row" (ba_amd/csrc/dist_plan.h), kout the panel width in tiles (0 = the engine's
 * choice for nblk).  Returns 0, or -1 if the layout does not exist for nranks. */
typedef struct {
  double factor_bytes;                         /* the whole factor: what a 1-D panel broadcast hands to every rank */
  double chain_recv_max, chain_recv_total;     /* per factorisation: busiest receiver / sum over ranks */
  double side_recv_max, side_recv_total;
  double chain_sent_total, side_sent_total;
  double recv_max;                             /* chain + side of the busiest receiver */
  double backward_allreduce_bytes;
  uint32_t messages_chain, messages_side, panels, ranks, classes, kout;
} ba_hip_dist_plan_stats_t;
int ba_hip_dist_plan_stats(uint32_t nblk, const uint8_t* nz_lower, int nranks, const char* layout, uint32_t kout,
                           ba_hip_dist_plan_stats_t* out);
/* Tile pattern of the factor as the engine holds it (nblk x nblk bytes, lower): for the accounting above.
 * With a pose ordering (ba_hip_set_pose_ordering) the pattern is in the order actually factorised. */
int ba_hip_get_factor_tile_pattern(ba_hip_engine* e, uint32_t nblk, uint8_t* nz_lower);
/* 1 if the next ba_hip_solve_gn will run the distributed solve, 0 if replicated / single. */
int ba_hip_solve_is_distributed(ba_hip_engine* e);

/* ---- fill-reducing pose ordering of the reduced camera solve (extension) ------------
 * The reference factorises S with Eigen's SimplicialLDLT, which applies an AMD ordering
 * (BundleAdjuster.cpp:752-761).  The engine factorises in the order of the optimisation
 * indices; with an ordering the poses are renumbered inside the engine at the next
 * ba_hip_finalize.  Every output indexed by the optimisation index (get_S, get_rhs,
 * get_delta_gn, get_step and the dumps built from them) stays in NATURAL order (active poses
 * in pose-id order): the caller never sees the internal one.  AUTO permutes tile-aligned groups
 * of G = lcm(PoseSize, 64) / PoseSize consecutive poses, keeps the partial last group and the
 * calibration unknowns last, and keeps the candidate ordering with the fewest tile products
 * (natural included).  Not available on sharded engines (all-reduce hook, collectives hook or
 * communicator): a mode other than NATURAL fails there, whichever of the two calls comes second. */
#define BA_HIP_ORDER_NATURAL 0 /* default: factorise in pose-id order */
#define BA_HIP_ORDER_AUTO 1    /* tile-aligned group ordering chosen by the engine */
#define BA_HIP_ORDER_USER 2    /* the permutation of ba_hip_set_pose_permutation */
typedef struct {
  int32_t mode;                    /* the mode the last finalize applied */
  int32_t candidate;               /* AUTO: 0 natural, 1 minimum degree + postorder, 2 minimum degree on pairs of
                                      groups + postorder, 3 nested dissection */
  uint32_t group_size;             /* G: poses per tile-aligned group */
  uint32_t num_groups;             /* ceil(active poses / G) */
  uint64_t tile_products_natural;  /* AUTO: model tile products of natural order and of the chosen one (the group */
  uint64_t tile_products_chosen;   /*       graph expanded to tiles; ba_hip_get_structure_stats has the exact count) */
  double host_ms;                  /* choosing the order on the host */
  double device_ms;                /* building the group graph on the device */
} ba_hip_ordering_stats;
/* Mode of the next ba_hip_finalize (one of BA_HIP_ORDER_*). */
int ba_hip_set_pose_ordering(ba_hip_engine* e, int mode);
/* The permutation of BA_HIP_ORDER_USER: opt_of_natural[i] = factorised position of the i-th active
 * pose; n must equal the active pose count at the next finalize.  Any permutation, aligned or not. */
int ba_hip_set_pose_permutation(ba_hip_engine* e, const uint32_t* opt_of_natural, uint32_t n);
/* What the last finalize applied: opt_of_natural (active pose count entries; may be NULL) and the
 * statistics (may be NULL). */
int ba_hip_get_pose_ordering(ba_hip_engine* e, uint32_t* opt_of_natural, ba_hip_ordering_stats* st);
/* The group graph AUTO chose from (CSR over the groups of natural order, symmetric, ascending): call with
 * NULL arrays for the sizes, then with ptr[num_groups + 1] and adj[num_edges]. */
int ba_hip_get_pose_group_graph(ba_hip_engine* e, uint32_t* ptr, uint32_t* adj, uint32_t* num_groups,
                                uint32_t* num_edges);

/* ---- marginal covariances (selected inverse of the reduced system) ------------------ */
/* Blocks of Sigma = S^-1 for the system the last ba_hip_solve_gn factorised (the last linearisation:
 * Huber weights, masks and pose-pose terms included — the system ba_hip_get_calibration_marginals
 * reads), in the tangent coordinates of the step, with a pose's layout of its entries of delta_p
 * (ba_hip_get_step).  Computed on the device from the factor by a selected inversion (the tiles of
 * S^-1 on the factor's tile pattern, kept in a store of their own; the factor, the kept S and the
 * calibration marginals are untouched).  Nothing is computed or allocated before the first request.
 *   - Pose ids and landmark ids are the caller's ids; an inactive pose or landmark is an error.
 *   - Masked parameters carry 1e6 on the diagonal of S: their variance reads ~1e-6.
 *   - Valid until the next ba_hip_linearize; after it every call is an error.
 *   - Pose orderings (BA_HIP_ORDER_AUTO / USER) are invisible: results are those of natural order.
 *   - Refused with the distributed solve; landmark blocks are also refused on sharded engines (each
 *     rank holds only its landmark shard), pose blocks are not (every rank holds the whole factor). */
typedef struct {
  double selinv_ms;              /* device time of the last selected inversion */
  double landmark_ms;            /* device time of the last landmark pass */
  uint64_t tile_products;        /* 64x64x64 tile products of the selected inverse: sum_J |R_J|^2 + tiles */
  uint64_t factor_tile_products; /* the factorisation's, for comparison (ba_hip_structure_stats) */
  double store_bytes;            /* bytes of the Sigma store */
  uint32_t store_tiles;          /* 64x64 tiles in it */
  uint32_t levels;               /* launch pairs of the schedule (levels of the elimination tree) */
} ba_hip_marginal_stats;
/* The selected inverse of the current factor; a no-op when it is already there. */
int ba_hip_compute_marginals(ba_hip_engine* e);
/* out: n x D x D row-major (D = PoseSize), the covariance of each pose. */
int ba_hip_get_pose_marginals(ba_hip_engine* e, uint32_t n, const uint32_t* pose_ids, double* out);
/* out: n x D x D, Cov(a_i, b_i) (rows: pose a_i, columns: pose b_i).  Available when all tiles of the
 * block lie in the factor's pattern — always for poses that share a landmark or a pose-pose residual;
 * otherwise an error. */
int ba_hip_get_pose_pair_marginals(ba_hip_engine* e, uint32_t n, const uint32_t* a_ids, const uint32_t* b_ids,
                                   double* out);
/* out: K x K, the calibration block of Sigma (K = ba_hip_set_calibration's unknowns), read from the store:
 * the same block ba_hip_get_calibration_marginals computes from the diagonal tiles. */
int ba_hip_get_calibration_block_marginals(ba_hip_engine* e, double* out);
/* out: n x LmSize x LmSize, Sigma_ll = V^-1 + V^-1 W^T Sigma_pp W V^-1 (the (l, l) block of the inverse of
 * the full poses + landmarks system) in the coordinates of delta_l (inverse depth for LmSize 1, x_w for
 * LmSize 3).  lm_ids NULL: every active landmark, by optimisation index (n = active landmark count).
 * An active landmark without observations has V = 0, which the guard of BundleAdjuster.cpp:431-439 turns
 * into 1e-6 I, and no W: its block is 1e6 I. */
int ba_hip_get_landmark_marginals(ba_hip_engine* e, uint32_t n, const uint32_t* lm_ids, double* out);
int ba_hip_get_marginal_stats(ba_hip_engine* e, ba_hip_marginal_stats* out);
/* Frees the Sigma store and the workspace of ba_hip_get_joint_marginals (also freed with the engine). */
int ba_hip_release_marginals(ba_hip_engine* e);

/* ---- leverages of projection residuals (hat blocks) -----------------------------------
 * For projection residual a with whitened Jacobian row block J_a = [A_a | B_a] (A_a: sqrt(w) dz_dx_meas at the
 * measuring pose, sqrt(w) dz_dx_ref at the reference pose (LmSize 1), sqrt(w) dz_dk at the calibration columns;
 * B_a = sqrt(w) dz_dlm; w = observation weight x Huber weight of the last linearisation; masked columns zero)
 * the 2 x 2 diagonal block of the hat matrix J (J^T J)^-1 J^T over all unknowns (poses, calibration, landmarks):
 *   H_aa = A Sigma A^T - sym2((sum_f A_f t_f) V^-1 B^T) + B Sigma_ll B^T,  t_f = sum_e Sigma_{p_f p_e} W_e,
 * with Sigma = S^-1 from the selected inverse (computed on demand) and Sigma_ll the landmark marginal.  From it:
 * redundancy 2 - tr H_aa, post-fit residual covariance I - H_aa, studentised residual r^T (I - H_aa)^-1 r,
 * innovation gate I + H_aa.  0 <= H_aa <= I; with projection residuals only and nothing masked the traces sum
 * to the number of unknowns.  With unary, binary or inertial residuals in the system the sum falls short by their
 * leverages: ba_hip_get_pose_pose_leverages serves those and completes the identity.
 *   - Preconditions of ba_hip_get_landmark_marginals: finalized, the factor of the last direct ba_hip_solve_gn
 *     (not PCG), not re-linearised since, not sharded or distributed.  Pose orderings are invisible.
 *   - Errors: an id that is no projection residual, NULL with n > 0, n != residual count with NULL ids, LmSize 0.
 *   - An inactive landmark drops B and the Schur part: H_aa = A Sigma A^T.  An inactive pose contributes no
 *     block.  An observation with no active incidence and an inactive landmark reads zero; w = 0 reads exactly
 *     zero.  An LmSize 1 observation taken from the landmark's reference pose itself carries no pose block (the
 *     listing rule of the reduced system): H_aa = B Sigma_ll B^T plus its calibration terms.
 *   - A repeated id returns the same bits twice, and an id's bits are those of the all-residuals call.
 *   - V^-1 does not enter as the explicit inverse the solve uses (its unstructured error of eps cond(V) |V^-1| is
 *     amplified by cond(V) again in B V^-1 B^T): the pass re-forms V = sum_a B_a^T B_a from the whitened dz_dlm
 *     with the same 1e-6 guard, factors it V = L L^T and works with L^-1.  A pivot that is not positive (a
 *     numerically singular V, which the solve's inverse does not survive either) is replaced by 1e-6.
 *   - Cost: a landmark with k incidences costs k^2 blocks of Sigma (2 k^2 beyond 64 observations) once per call,
 *     however many of its residuals the call asks for, plus O(1) blocks per residual.  Asking for the residuals of
 *     one landmark in separate calls pays the k^2 each time (k^3 for a whole track): ask for them together.
 *   - Nothing is allocated on the device before the first request and nothing is kept there between requests
 *     (the host keeps the sorted position of every residual id until the next ba_hip_finalize). */
/* out: n x 4 (row-major 2 x 2, bitwise symmetric) per ACCEPTED projection residual id; residual_ids NULL:
 * every residual in residual-id order (n = their count). */
int ba_hip_get_projection_leverages(ba_hip_engine* e, uint32_t n, const uint32_t* residual_ids, double* out);
typedef struct {
  double device_ms;      /* device time of the last leverage pass (events) */
  uint64_t block_reads;  /* blocks of Sigma it read: v^2 per landmark with v incidences (twice beyond 64
                            observations), c^2 per residual with c blocks in A */
  uint32_t residuals, landmarks;  /* residuals served, landmarks they belong to */
} ba_hip_leverage_stats;
/* The figures of the last successful ba_hip_get_projection_leverages (zeros before the first). */
int ba_hip_get_leverage_stats(ba_hip_engine* e, ba_hip_leverage_stats* out);

/* ---- leverages of unary, binary and inertial residuals (hat blocks) -----------------------
 * Residual i of a kind couples pose p1 and (binary, inertial) p2.  With
 *   J_i       = [dz1 | dz2], R x 2 D: the UNWHITENED Jacobians of the residual in its own raw coordinates (R = 6 for
 *               unary and binary residuals, PoseSize for inertial ones); the column of a masked parameter and the
 *               block of an inactive pose are zero,
 *   Lambda_i    the EFFECTIVE information, for which J_i^T Lambda_i J_i is what the residual added to S:
 *                 unary     cov_inv x scale (ba_hip_get_unary_scales: the compounded Huber weights),
 *                 binary    weight x cov_inv_sqrt^T cov_inv_sqrt, with cov_inv_sqrt as the caller supplied it (the
 *                           engine's internal copy of cov_inv is unweighted and is NOT Lambda_i),
 *                 inertial  cov_inv x Huber factor of the last linearisation,
 *   Sigma_ee    the block of Sigma = S^-1 over the rows of p1, p2 (selected inverse, computed on demand),
 * the call serves C_i = J_i Sigma_ee J_i^T (the covariance of the predicted residual, bitwise symmetric), Lambda_i
 * as used, and the leverage l_i = tr(C_i Lambda_i).  With any square root Lambda = G G^T: the whitened hat block
 * G^T C G (0 <= . <= I), redundancy R_eff - l_i, post-fit residual covariance Lambda^-1 - C, studentised statistic
 * r^T (Lambda^-1 - C)^-1 r, innovation gate Lambda^-1 + C.  Over all residual kinds, nothing masked and every
 * unknown touched: sum tr H_aa (projection) + sum l_i = number of unknowns (dense priors of
 * ba_hip_set_dense_priors are not served; the identity holds for systems without them).
 *   - Preconditions of the pose getters: finalized, the factor of the last direct ba_hip_solve_gn (not PCG), not
 *     re-linearised since, not the distributed solve (replicated sharded engines are served).  LmSize 0 and every
 *     PoseSize work; pose orderings are invisible.
 *   - Errors: an unknown kind, an id beyond the kind's count, n != the kind's count with NULL ids, all three outputs
 *     NULL with n > 0, a pose pair whose block of Sigma is outside the factor's pattern (not possible for poses a
 *     residual couples; reported, never returned as NaN).
 *   - A binary residual with use_rotation = 0 has zero rows 3..5 in J: C is zero there, info is not.
 *   - A residual whose poses are all inactive reads zero in cov and leverage.
 *   - A repeated id returns the same bits twice, and an id's bits are those of the all-residuals call.
 *   - Nothing is allocated on the device before the first request and nothing is kept there between requests
 *     beyond the Sigma store (ba_hip_release_marginals). */
#define BA_HIP_RES_UNARY 0
#define BA_HIP_RES_BINARY 1
#define BA_HIP_RES_IMU 2
/* cov, info: n x 225 (15 x 15 row-major, zero outside the residual's R x R block), either may be NULL;
 * leverage: n, may be NULL; ids NULL: every residual of the kind in id order (n = their count). */
int ba_hip_get_pose_pose_leverages(ba_hip_engine* e, int kind, uint32_t n, const uint32_t* ids, double* cov,
                                   double* info, double* leverage);
typedef struct {
  double device_ms;       /* device time of the last pass (events) */
  uint64_t sigma_blocks;  /* D x D blocks of Sigma it read: (live poses)^2 per residual */
  uint32_t residuals;     /* residuals served */
  uint32_t kind;          /* their kind */
} ba_hip_pose_pose_leverage_stats;
/* The residuals of a kind in the engine (what n must be with NULL ids); 0 for an unknown kind. */
uint32_t ba_hip_num_pose_pose_residuals(const ba_hip_engine* e, int kind);
/* The figures of the last ba_hip_get_pose_pose_leverages that passed its checks (zeros before the first). */
int ba_hip_get_pose_pose_leverage_stats(ba_hip_engine* e, ba_hip_pose_pose_leverage_stats* out);

/* ---- joint covariance of an arbitrary pose set (no selected inverse) ------------------
 * The M x M block of Sigma = S^-1 over the rows of the poses pose_ids (and, with include_calibration, the K
 * calibration rows after them), M = n D + (include_calibration ? K : 0): block (i, j) of out (row-major) is
 * Cov(pose_ids[i], pose_ids[j]) in the caller's order, in the coordinates and with the Sigma of the getters
 * above (masked parameters read ~1e-6, pose orderings are invisible).  Any set of active poses is served,
 * whether or not the factor's tile pattern couples them: with S = L D L^T the block is Y^T D Y, Y = L^-1 E for
 * the unit columns E of the requested rows, a forward substitution over the tile rows on the elimination-tree
 * paths from the requested tiles to the root (the reach) and a Gram product.  The selected inverse is neither
 * computed nor allocated, ba_hip_get_marginal_stats is untouched; the call reads the factor only.  out is
 * bitwise symmetric and two calls give the same bits.
 *   - Preconditions of the pose getters: finalized, the factor of the last direct ba_hip_solve_gn, not
 *     re-linearised since, not the distributed solve (replicated sharded engines are served).
 *   - Errors: an inactive pose, a repeated id, include_calibration without calibration unknowns, no column at
 *     all, M > BA_HIP_JOINT_MAX_COLUMNS, NULL arguments.
 *   - The workspace (the Y panels and the partial tiles) is allocated by the first request, reused, and freed
 *     by ba_hip_release_marginals and with the engine. */
#define BA_HIP_JOINT_MAX_COLUMNS 512
typedef struct {
  double solve_ms;          /* device time of the forward substitution (events) */
  double gram_ms;           /* device time of the Gram product and its combine */
  double workspace_bytes;   /* device bytes the joint path holds */
  uint64_t tile_products;   /* 64x64x64 products: (sum_{I in reach} |row(I) n reach| + |reach|) per 64 columns */
  uint32_t columns;         /* M */
  uint32_t reach_tiles;     /* tile rows visited */
  uint32_t levels;          /* launch pairs of the substitution */
  uint32_t reserved;
} ba_hip_joint_marginal_stats;
int ba_hip_get_joint_marginals(ba_hip_engine* e, uint32_t n, const uint32_t* pose_ids, int include_calibration,
                               double* out);
/* The figures of the substitution and the Gram product of the last successful ba_hip_get_joint_marginals or
 * ba_hip_get_joint_state_marginals (zeros before the first). */
int ba_hip_get_joint_marginal_stats(ba_hip_engine* e, ba_hip_joint_marginal_stats* out);

/* ---- solves with the kept factor: X = S^-1 B for a caller's right-hand sides ----------
 * S is the reduced system that the last direct ba_hip_solve_gn factorised (S = L D L^T, tile-sparse, left on the
 * device); B holds m columns of the caller's own.  Both passes of the substitution run over every tile row, by
 * levels of the factor's pattern, on the matrix cores.
 *   - n = ba_hip_num_pose_params + ba_hip_num_calib_params.  B and X are n x m, row-major, on the host; their rows
 *     are in the order and coordinates of ba_hip_get_delta_gn (natural pose order whatever the pose ordering, the
 *     calibration rows last).  X may be B.
 *   - Preconditions of ba_hip_get_joint_marginals: a direct solve since the last linearisation, not the PCG
 *     solver, not the distributed solve, no stand-alone solve since.  Replicated sharded engines are served.
 *   - Refused with a message: m == 0, m > BA_HIP_FACTOR_SOLVE_MAX_COLUMNS, NULL arguments.
 *   - Reads the factor only: the Sigma store, its validity and the statistics of the other getters stay untouched.
 *     No atomics: two calls give the same bits.
 *   - The workspace is allocated by the first call, grown on demand and freed by ba_hip_release_marginals. */
#define BA_HIP_FACTOR_SOLVE_MAX_COLUMNS 512
typedef struct {
  double forward_ms;        /* Y = L^-1 B */
  double backward_ms;       /* X = L^-T D Y */
  double workspace_bytes;   /* device bytes the solve holds */
  uint64_t tile_products;   /* 64 x 64 x 64 products of both passes */
  uint32_t columns;         /* m */
  uint32_t tiles;           /* tile rows of the factor */
  uint32_t forward_levels;  /* launch pairs of the forward pass */
  uint32_t backward_levels; /* ... of the backward pass */
} ba_hip_factor_solve_stats;
int ba_hip_factor_solve(ba_hip_engine* e, uint32_t m, const double* B, double* X);
/* The figures of the last successful ba_hip_factor_solve or ba_hip_tile_factor_solve (zeros before the first). */
int ba_hip_get_factor_solve_stats(ba_hip_engine* e, ba_hip_factor_solve_stats* out);

/* ---- weakest modes: the eigenpairs of S of smallest magnitude ---------------------------
 * Which directions of the problem are weakly determined (a free scale, yaw about gravity, a bias ...): the k
 * eigenpairs of the S that the last direct ba_hip_solve_gn factorised whose eigenvalues are smallest in magnitude,
 * by block inverse iteration with Rayleigh-Ritz on min(64, n) vectors.  Only S^-1 is needed (ba_hip_factor_solve on
 * panels that stay on the device), so the in-place factorisation does not stand in the way.
 *   - 1 <= k <= min(32, n).  eigenvalues: k values by ascending magnitude; with negative pivots S is indefinite and
 *     the sign is reported.  modes: k x n row-major, each row a unit vector in the rows and coordinates of
 *     ba_hip_factor_solve (6 or more consecutive entries per active pose in natural order, calibration last).
 *   - Options: NULL, or a zero field, takes the default: tolerance 1e-8, max_iterations 50, seed 1.  Pair i has
 *     converged when |S^-1 v_i - theta_i v_i| <= tolerance |theta_i|, theta_i = 1 / lambda_i.
 *   - Returns 0 also when the cap is reached with converged < k (ba_hip_get_mode_stats): eigenvalues and modes are
 *     then the last Ritz pairs, not converged ones.
 *   - The start block is counter based (splitmix64 of seed, row and column, stated in factorsolve.h), no atomics:
 *     a second call returns the same bits.
 *   - Preconditions, refusals and workspace as for ba_hip_factor_solve; besides k == 0, k > min(32, n), NULL. */
typedef struct {
  double tolerance;
  uint32_t max_iterations;
  uint32_t seed;
  uint32_t reserved[3];
} ba_hip_mode_options;
typedef struct {
  double solve_ms;          /* applying S^-1, all iterations (host clock around the drained stream) */
  double ortho_ms;          /* orthonormalisation, Gram products and host eigenproblems included */
  double residual_max;      /* largest |S^-1 v - theta v| / |theta| over the k pairs at return */
  double workspace_bytes;
  uint32_t iterations;
  uint32_t converged;       /* pairs among the k that met the tolerance */
  uint32_t block;           /* vectors iterated: min(64, n) */
  uint32_t reserved;
} ba_hip_mode_stats;
int ba_hip_get_weakest_modes(ba_hip_engine* e, uint32_t k, const ba_hip_mode_options* o, double* eigenvalues,
                             double* modes);
/* The figures of the last successful ba_hip_get_weakest_modes (zeros before the first). */
int ba_hip_get_mode_stats(ba_hip_engine* e, ba_hip_mode_stats* out);

/* ---- joint covariance of a mixed set of poses, calibration and landmarks (cross blocks) ----
 * The M x M block of the inverse of the full system [[U, W], [W^T, V]] over the requested parameters,
 * M = n_poses D + (include_calibration ? K : 0) + n_landmarks LmSize; columns in that order: the poses in the
 * caller's order, the calibration rows, the landmarks in the caller's order.  Poses and calibration use the
 * coordinates of delta_p, landmarks those of delta_l; orderings are invisible.  It holds the pose-landmark cross
 * blocks Cov(p, l) = -Sigma_pp W_l V_l^-1 and the landmark-landmark blocks V_l^-1 W_l^T Sigma_pp W_l' V_l'^-1
 * (+ V_l^-1 when l = l'), which no other getter serves.  Same substitution and Gram product as
 * ba_hip_get_joint_marginals, started from the columns [E | -W_l V_l^-1] instead of unit columns alone; with
 * n_landmarks == 0 the result is bit for bit that of ba_hip_get_joint_marginals.  The selected inverse is
 * neither computed nor allocated, ba_hip_get_marginal_stats is untouched.  out is bitwise symmetric and two calls
 * give the same bits.
 *   - Preconditions of ba_hip_get_joint_marginals; with n_landmarks > 0 sharded engines are refused as by
 *     ba_hip_get_landmark_marginals.
 *   - Errors: an inactive or out-of-range pose or landmark, a repeated pose or landmark id, n_landmarks > 0 with
 *     LmSize 0, include_calibration without calibration unknowns, M == 0, M > BA_HIP_JOINT_MAX_COLUMNS, NULL.
 *   - An active landmark without observations reads 1e6 I with exactly zero cross blocks (the convention of
 *     ba_hip_get_landmark_marginals).
 *   - The workspace is the joint path's (ba_hip_release_marginals). */
typedef struct {
  double rhs_ms;              /* device time of the right-hand-side pass (events) */
  double seed_ms;             /* device time of the seed pass */
  uint64_t incidences;        /* valid incidences scattered into the landmark columns */
  uint32_t landmark_columns;  /* n_landmarks LmSize */
  uint32_t seed_tiles;        /* tile rows the landmark columns touch */
} ba_hip_joint_state_stats;
int ba_hip_get_joint_state_marginals(ba_hip_engine* e, uint32_t n_poses, const uint32_t* pose_ids,
                                     int include_calibration, uint32_t n_landmarks, const uint32_t* lm_ids,
                                     double* out);
/* The figures of the last successful ba_hip_get_joint_state_marginals (zeros before the first). */
int ba_hip_get_joint_state_stats(ba_hip_engine* e, ba_hip_joint_state_stats* out);

/* ---- sliding-window marginalisation and dense pose priors (extension) ----------------
 * Conventions are the engine's: S delta = rhs (rhs_p_sc), ApplyUpdate(delta) moves a pose by
 * exp_decoupled(T, -delta_6), v -= delta_v, b -= delta_b, and the Gauss-Newton model of the system at its
 * linearisation state is m(delta) = E - 2 rhs^T delta + delta^T S delta.
 *
 * Dense prior residual on poses p_1 .. p_k, holding (x0, H, b, c): d_i(x) is the delta ApplyUpdate would need
 * to take x0_i to x_i (d_t = t0 - t, d_w = log(q^-1 q0), d_v = v0 - v, d_b = b0 - b; zero at x0), and
 *     E_p(x) = c - 2 b^T d + d^T H d.
 * Linearised at x it adds J_d^T H J_d to S and J_d^T (b - H d) to rhs_p / rhs_p_sc (J_d = dd/ddelta,
 * block-diagonal, the identity at x0); masked parameters are skipped as for every pose-pose residual; no robust
 * weight.  E_p is folded into ba_errors.unary_error (linearize and eval_residuals) and the dogleg denominator
 * j_rhs_sq gains (J_d g)^T H (J_d g).  Inactive poses are constants.  The priors are applied after the unary,
 * binary and inertial residuals, in prior order, so sums stay deterministic.
 *
 * Marginalisation of poses M and landmarks L out of the last linearisation into a prior on their blanket B:
 *   absorbed: every projection residual of a landmark in L; every unary residual on a pose in M; every binary
 *             and inertial residual with a pose in M; every dense prior covering a pose in M;
 *   dropped:  the projection residuals of landmarks NOT in L measured by a pose in M (counted);
 *   B:        the active poses outside M that appear in an absorbed residual, sorted by pose id.
 * With S^a, rhs^a, E^a the absorbed part of the system with L eliminated (E^a: the absorbed residuals' share of
 * the error sums, less sum_l rhs_l^T V_l^-1 rhs_l):
 *   H = S^a_BB - S^a_BM (S^a_MM)^-1 S^a_MB,  b = rhs^a_B - S^a_BM (S^a_MM)^-1 rhs^a_M,
 *   c = E^a - rhs^a_M^T (S^a_MM)^-1 rhs^a_M,  x0 = the state of every blanket pose.
 * A masked parameter of M keeps a unit pivot; one of B has zero rows and columns in H.  The system "everything
 * not absorbed, plus the prior", linearised at the same state, is then exactly the full system with M and L
 * eliminated.  Refused (error, the engine stays usable): M empty, duplicate, unknown or inactive; L unknown,
 * duplicate, inactive, or non-empty with LmSize 0; an active landmark anchored in M (LmSize 1) missing from L;
 * calibration unknowns; sharded engines and the distributed solve; no linearisation of the current state (a step,
 * rollback, new masks or begin_solve since); |M| * PoseSize > 128; |B| * PoseSize > 4096; S^a_MM not positive
 * definite (a pivot d_j <= tol * S_jj, tol = pivot_rel_tolerance or 1e-10 when that is 0): returns
 * BA_HIP_FACTORIZATION_ERROR. */
typedef struct {
  uint32_t blanket_poses;
  uint32_t absorbed_projection, absorbed_unary, absorbed_binary, absorbed_inertial, absorbed_priors;
  uint32_t dropped_projection, reserved;
  double device_ms;   /* the marginalisation kernels, assembly to the last output */
  double host_ms;     /* the whole call: plan, uploads, kernels, read-back */
} ba_hip_marginalization_stats;
/* n priors, CSR ptr[n + 1] over pose_ids (caller's ids, no pose twice in a prior); per covered pose x0_16 = its
 * 16-double state t(3) q(4) v(3) b(6); per prior H (kD x kD row-major, k = its pose count, D = PoseSize), b (kD),
 * c (1), concatenated in prior order.  H is read as symmetric: (H + H^T) / 2 is kept.  Structural: call before ba_hip_finalize (n = 0 removes them).  Every tile
 * of a prior's blocks joins the factor's pattern and the pose ordering's group graph.  Refused with calibration
 * unknowns (at finalize) and on sharded engines (at linearize). */
int ba_hip_set_dense_priors(ba_hip_engine* e, uint32_t n, const uint32_t* ptr, const uint32_t* pose_ids,
                            const double* x0_16, const double* H, const double* b, const double* c);
/* E_p of every prior at the last ba_hip_linearize or ba_hip_eval_residuals; n = the prior count. */
int ba_hip_get_prior_errors(ba_hip_engine* e, uint32_t n, double* out);
/* Computes the prior of marginalising m_ids / l_ids into an engine-owned store.  A successful call replaces
 * the stored result; a refused call leaves it, a failed computation (BA_HIP_FACTORIZATION_ERROR) clears it.
 * stats may be NULL. */
int ba_hip_marginalize(ba_hip_engine* e, uint32_t nm, const uint32_t* m_ids, uint32_t nl, const uint32_t* l_ids,
                       ba_hip_marginalization_stats* stats);
/* The stored result: blanket_ids (|B|), x0_16 (|B| x 16), H (|B|D x |B|D, bitwise symmetric), b (|B|D), c (1);
 * any pointer may be NULL. */
int ba_hip_get_marginalization(ba_hip_engine* e, uint32_t* blanket_ids, double* x0_16, double* H, double* b, double* c);
/* Frees the store (also freed with the engine). */
int ba_hip_release_marginalization(ba_hip_engine* e);

/* ---- iterative reduced solve: block-Jacobi preconditioned conjugate gradients (extension) ----------
 * The second solver behind ba_hip_solve_gn (inexact Gauss-Newton; Agarwal et al., "Bundle adjustment in the
 * large"): S delta = rhs is solved by conjugate gradients from x0 = 0 on the tiles of S's own pattern (no fill),
 * preconditioned by the diagonal blocks of S — one PoseSize x PoseSize block per active pose in the order the
 * engine factorises, one K x K block for the calibration unknowns.  FP64, no atomics: two solves of the same
 * system give the same bits.  The default stays the direct tile-sparse LDL^T.
 *
 * Stopping rule: when the recurrence reports ||r|| <= rel_tolerance * ||rhs|| the residual rhs - S x is recomputed
 * and only that TRUE residual ends the solve with converged = 1; if it fails, the solve continues from the
 * recomputed residual (residual_replacements counts these).  Reaching max_iterations is not an error: ba_hip_solve_gn
 * returns 0 with converged = 0 (CG iterates from x0 = 0 are descent directions of the model).  A breakdown — p.Sp <= 0,
 * a non-finite scalar, a preconditioner block that is not positive definite — returns BA_HIP_FACTORIZATION_ERROR
 * and leaves the last iterate whose scalars were finite (zeros if none) in delta_gn.  The host reads the device's
 * state every check_every passes only; alpha, beta and the decisions are formed on the device.
 *
 * The mode is not structural: it may change between two iterations without ba_hip_finalize.  After a PCG solve
 *   - A still holds S: ba_hip_get_S works without keep_reduced_system, and ba_hip_check_solve runs on S itself
 *     (its dense two-pass product shares no code with the solver's tile product: an independent check of
 *     rel_residual_true);
 *   - there is no factor: ba_hip_compute_marginals, the marginal getters and ba_hip_get_calibration_marginals
 *     refuse with a message that names the solver.  ba_hip_marginalize reads the linearisation (factor rows,
 *     pose-pose blocks), not the factor, and works as before;
 *   - pose orderings, calibration unknowns, dense priors, LmSize 0 and the dogleg path work unchanged (outputs
 *     stay in natural order; delta_gn is simply inexact).
 * Sharded engines (all-reduce hook, collectives hook, communicator) refuse PCG, whichever call comes second. */
#define BA_HIP_SOLVER_DIRECT 0   /* default: tile-sparse LDL^T */
#define BA_HIP_SOLVER_PCG    1   /* preconditioned conjugate gradients on S (block-Jacobi; optionally two-level) */
typedef struct {
  double rel_tolerance;
  uint32_t max_iterations;   /* CG steps; 0 = the number of unknowns */
  uint32_t check_every;      /* passes between two reads of the device state; 0 = the engine's choice */
  uint32_t coarse_aggregate; /* 0 = block-Jacobi alone; g >= 1 = two-level preconditioner, aggregates of g poses (below) */
  uint32_t reserved[2];
} ba_hip_pcg_options;
typedef struct {
  uint32_t iterations, converged, residual_replacements;
  uint32_t breakdown;               /* 0 none, 1 p.Sp <= 0, 2 non-finite scalar, 3 preconditioner block not PD,
                                     * 4 coarse matrix not PD (two-level preconditioner) */
  double rel_residual_recurrence;   /* ||r|| / ||rhs|| of the recurrence at the end */
  double rel_residual_true;         /* ... of the last recomputed rhs - S x (0 if none was formed) */
  double rhs_norm;
  double solve_ms;                  /* the whole solve, preconditioner included */
  double spmv_ms;                   /* mean device time of one product q = S p (sampled once per check_every) */
  double precond_ms;                /* gathering and inverting the blocks */
  uint64_t tiles_read_per_spmv;     /* lower tiles of S's pattern */
  double bytes_read_per_spmv;       /* tiles + partial-sum slots + vectors */
} ba_hip_pcg_stats;
/* mode: BA_HIP_SOLVER_*; o: NULL with DIRECT (and with PCG: rel_tolerance 1e-6, the defaults above). */
int ba_hip_set_reduced_solver(ba_hip_engine* e, int mode, const ba_hip_pcg_options* o);
/* Statistics of the last ba_hip_solve_gn; an error if that solve was direct (or skipped). */
int ba_hip_get_pcg_stats(ba_hip_engine* e, ba_hip_pcg_stats* out);
/* Two-level preconditioner (ba_hip_pcg_options.coarse_aggregate = g >= 1; 0 keeps the block-Jacobi solver bit for
 * bit): M^-1 = M_bj^-1 + Z (Z^T S Z)^-1 Z^T.  Z sums parameter d of the g consecutive active poses of an aggregate
 * (pose-id order, whatever the pose ordering; the last aggregate may be short) into coarse unknown (aggregate, d);
 * the K calibration unknowns are K coarse unknowns of their own.  In ba_hip_pcg_solve an aggregate is g consecutive
 * preconditioner blocks; a short last block feeds the leading coarse parameters of its aggregate.  When
 * D ceil(Pact / g) + K would exceed BA_HIP_PCG_COARSE_MAX the engine raises g to the smallest value that fits
 * (aggregate_used): a request never fails for size.  The coarse matrix and its explicit inverse are formed once per
 * solve; a pivot <= 0 in its factorisation is breakdown 4 (BA_HIP_FACTORIZATION_ERROR, delta_gn zero). */
#define BA_HIP_PCG_COARSE_MAX 1024
typedef struct {
  uint32_t aggregate_used, coarse_unknowns, aggregates, reserved;
  double setup_ms;                  /* assembling and inverting the coarse matrix */
  double apply_ms;                  /* the two coarse launches of one pass, mean over the sampled passes */
  double coarse_bytes;              /* device memory of the coarse matrices and vectors */
} ba_hip_pcg_coarse_stats;
/* Of the last ba_hip_solve_gn or ba_hip_pcg_solve; an error if that solve did not use the coarse space. */
int ba_hip_get_pcg_coarse_stats(ba_hip_engine* e, ba_hip_pcg_coarse_stats* out);
/* Test tap: the coarse matrix and its inverse of the last two-level solve, row-major nc x nc (nc = coarse_unknowns);
 * either pointer may be NULL. */
int ba_hip_get_pcg_coarse(ba_hip_engine* e, uint32_t nc, double* C, double* Cinv);

/* ---- panel PCG: S^-1 applied to a block of columns after a PCG solve (extension) ----------------------
 * After a PCG solve there is no factor, but A still holds S.  ba_hip_pcg_panel_solve_system computes X = S^-1 B for
 * 1 <= m <= BA_HIP_PCG_PANEL_MAX_COLUMNS right-hand sides by m INDEPENDENT block-Jacobi PCG recurrences run in
 * lock-step (not block CG: no m x m systems, dependent columns are no problem).  Every column has the stopping
 * rule, the true-residual verification, the residual replacement and the breakdown codes of the solver above, its
 * own alpha and beta and its own iteration count; a finished column is frozen while the others go on.  Only the
 * tiles of S are shared: a pass reads them once per block of 64 columns and multiplies on the FP64 matrix cores.
 * FP64, no atomics, fixed summation order: a second call returns the same bits, and column j of X has the same bits
 * whatever the other columns hold and wherever in B it sits.
 *   B, X   n x m row-major (host), n = pose + calibration parameters; rows in the order and coordinates of
 *          ba_hip_factor_solve (natural pose order under every pose ordering, the calibration rows last).
 *   o      rel_tolerance in (0, 1), max_iterations and check_every as above; coarse_aggregate must be 0 (the coarse
 *          space is not available in panel solves).
 * Precondition: the last ba_hip_solve_gn ran PCG and the system has not been linearised since.  Refused with a
 * message otherwise, and for a direct solver, a sharded engine, m == 0, m > the limit, NULL arguments and
 * coarse_aggregate != 0.  Reads A only: delta_gn, the statistics of the last ba_hip_solve_gn and every validity
 * flag of the engine stay as they are.
 * Returns 0 when no column broke down (columns that ran into max_iterations are reported per column, not as an
 * error) and BA_HIP_FACTORIZATION_ERROR when some column did; X then holds every column's last finite iterate. */
#define BA_HIP_PCG_PANEL_MAX_COLUMNS 512
int ba_hip_pcg_panel_solve_system(ba_hip_engine* e, uint32_t m, const double* B, double* X, const ba_hip_pcg_options* o);
/* The block of S^-1 that ba_hip_get_joint_marginals returns, in the same layout (the poses in the caller's order,
 * the calibration rows last), computed without a factor: G = E^T (S^-1 E) by the panel solve on unit columns,
 * returned as (G + G^T) / 2.  Preconditions and refusals of ba_hip_pcg_panel_solve_system; the accuracy is that of
 * the options' rel_tolerance (relative error about cond(S) * rel_tolerance). */
int ba_hip_get_joint_marginals_pcg(ba_hip_engine* e, uint32_t n, const uint32_t* pose_ids, int include_calibration,
                                   const ba_hip_pcg_options* o, double* out);
typedef struct {
  uint32_t columns, column_blocks;  /* m, ceil(m / 64) */
  uint32_t passes;                  /* passes enqueued until every column was done (or the cap) */
  uint32_t converged, capped, broken_down;   /* columns; they add up to `columns` */
  double max_rel_residual_true;     /* the largest ||b_j - S x_j|| / ||b_j|| over the converged and capped columns */
  double solve_ms;                  /* the whole call on the device, block inverses included */
  double spmm_ms;                   /* mean device time of one product Q = S P (sampled once per check_every) */
  double tile_products_per_pass;    /* 64 x 64 x 64 products of one pass (all column blocks) */
  double bytes_read_per_product;    /* of one product Q = S P: tiles, panel tiles and partial-tile slots */
  double workspace_bytes;           /* device memory of the panel solver */
} ba_hip_pcg_panel_stats;
/* Of the last panel solve (either entry point above, or the test tap). */
int ba_hip_get_pcg_panel_stats(ba_hip_engine* e, ba_hip_pcg_panel_stats* out);
/* The per-column record of the last panel solve; m must be its column count; every pointer may be NULL.
 * breakdown: the codes of ba_hip_pcg_stats. */
int ba_hip_get_pcg_panel_columns(ba_hip_engine* e, uint32_t m, uint32_t* iterations, uint32_t* converged,
                                 uint32_t* breakdown, double* rel_residual_true);

/* ---- stand-alone kernels exposed for tests and benchmarks ------------------------- */
/* The PCG solver on an SPD system given by its LOWER triangle (row-major n x n, host memory); `block`: size of the
 * preconditioner's diagonal blocks (1 .. 16; the last block is shorter when it does not divide n).  The tile
 * pattern is that of the nonzeros of a_lower.  Returns 0 or BA_HIP_FACTORIZATION_ERROR as described above. */
int ba_hip_pcg_solve(ba_hip_engine* e, uint32_t n, const double* a_lower, const double* b, uint32_t block,
                     const ba_hip_pcg_options* o, double* x, ba_hip_pcg_stats* stats);
/* Test tap of the panel PCG: X = A^-1 B (n x m row-major, host) on the system of ba_hip_pcg_solve — lower triangle,
 * pattern of its nonzeros, one block size — by the kernels of ba_hip_pcg_panel_solve_system.  stats may be NULL.
 * Returns and lifecycle effects as ba_hip_pcg_solve; the per-column record is read with ba_hip_get_pcg_panel_columns. */
int ba_hip_pcg_panel_solve(ba_hip_engine* e, uint32_t n, const double* a_lower, uint32_t m, const double* B, uint32_t block,
                           const ba_hip_pcg_options* o, double* X, ba_hip_pcg_panel_stats* stats);
/* Dense Cholesky solve of an SPD system given by its LOWER triangle (row-major n x n,
 * host memory): x = A^-1 b.  Runs the same kernels ba_hip_solve_gn uses. */
int ba_hip_dense_solve(ba_hip_engine* e, uint32_t n, const double* a_lower, const double* b, double* x);
/* The direct tile-sparse L D L^T solve (the kernels of ba_hip_solve_gn) of a symmetric system given by its LOWER
 * triangle (row-major n x n, host memory), with a caller-supplied pattern of 64x64 tiles.  nt = max(1, ceil(n / 64)).
 *   tile_map   nt x nt bytes, row-major; byte (i, k), k <= i, nonzero = tile (i, k) of the matrix may hold nonzeros
 *              (a superset of the true pattern is fine; the diagonal tiles always count).  A nonzero entry in a
 *              tile the map leaves out is refused.  NULL: the pattern of the nonzeros of a_lower.
 *   x          n doubles, the solution.
 *   nz_factor  (may be NULL) nt x nt bytes: the lower tile pattern of L after symbolic elimination.
 *   factor, linvT, dsgn  (each may be NULL) the kept factor as the engine holds it: the (64 nt) x (64 nt) row-major
 *              storage after the factorisation (L's tiles below the diagonal tiles; rows >= n are identity padding),
 *              nt row-major 64x64 tiles L_JJ^-T, and the 64 nt pivot signs.
 * Returns 0 or BA_HIP_FACTORIZATION_ERROR.  The engine's scene is left alone, but the factor kept by the last
 * ba_hip_solve_gn is gone afterwards: the marginal covariances are refused until the next ba_hip_solve_gn. */
int ba_hip_tile_solve(ba_hip_engine* e, uint32_t n, const double* a_lower, const double* b, const uint8_t* tile_map,
                      double* x, uint8_t* nz_factor, double* factor, double* linvT, double* dsgn);
/* Test tap of ba_hip_factor_solve: the factorisation of ba_hip_tile_solve on (a_lower, tile_map), then X = A^-1 B
 * (n x m row-major, host; m <= BA_HIP_FACTOR_SOLVE_MAX_COLUMNS) by the substitution kernels of ba_hip_factor_solve
 * on the factor it leaves.  Returns and lifecycle effects as ba_hip_tile_solve. */
int ba_hip_tile_factor_solve(ba_hip_engine* e, uint32_t n, const double* a_lower, const uint8_t* tile_map, uint32_t m,
                             const double* B, double* X);
/* exact k-th smallest (0-based) of n non-negative doubles — the device selection behind
 * the Huber sigma (std::nth_element at floor(N/2), BundleAdjuster.cpp:1356-1358) */
int ba_hip_select_kth(ba_hip_engine* e, uint32_t n, const double* values, uint32_t k, double* out);

/* ---- Landmark triangulation and per-landmark refinement, poses held fixed (ba_amd/csrc/triang.h) ----
 * With the poses fixed every landmark is a least-squares problem of its own (3 parameters with LmSize 3, the inverse
 * depth along the reference ray with LmSize 1).  One launch (k_triang.hip) gives each selected landmark a closed-form
 * linear estimate from its observations and refines it by Levenberg-Marquardt to convergence, on the pose state the
 * engine holds, with the cameras of the rig (pinhole and FOV), the per-pose intrinsics when set, and the original
 * weights of the observations.  The active flag of a landmark is not consulted: the id list decides.
 * LmSize 1 reads the ray as unit(T_sw(ref) x_w): a landmark uploaded as a pure direction (w = 0) is valid input.
 * Uses: landmarks uploaded as directions only; re-triangulation after tracking; with write_back = 0 an audit of the
 * map (parallax, cheirality and cost per landmark) that changes nothing.
 * Placement: after ba_hip_finalize, outside a Solve (before ba_hip_begin_solve or after ba_hip_end_solve).  Refused with
 * LmSize 0, with calibration unknowns, on a sharded or hooked engine and between ba_hip_begin_solve and ba_hip_end_solve.
 * With write_back the accepted coordinates replace the landmarks' (every other landmark keeps its bits), x_s is
 * re-derived (LmSize 1) and the call then counts as a ba_hip_begin_solve for everything the device holds: the
 * linearisation and the cached errors are dropped, the kept factor stays readable.  With write_back = 0 nothing the
 * engine holds changes.  Two identical calls return identical bits.  The work space is allocated by the first call and
 * freed by ba_hip_release_marginals. */
enum {
  BA_HIP_TRI_OK = 0,             /* converged; written back */
  BA_HIP_TRI_NOT_CONVERGED = 1,  /* iteration limit reached; written back if the cost fell (with linear_init: did not rise) */
  BA_HIP_TRI_TOO_FEW_VIEWS = 2,  /* fewer than 2 observations, or none with a baseline; not written */
  BA_HIP_TRI_LOW_PARALLAX = 3,   /* below min_parallax; not written */
  BA_HIP_TRI_BEHIND_CAMERA = 4,  /* depth <= 0 in an observing sensor at the starting point; not written */
  BA_HIP_TRI_FAILED = 5          /* non-finite result; not written */
};
typedef struct {
  int32_t linear_init;       /* 1 (default): start from the closed-form estimate; 0: from the coordinates held */
  int32_t max_iterations;    /* refinement steps per landmark, 0..64; default 20; 0 = linear estimate only */
  int32_t write_back;        /* 1 (default): accepted landmarks get the new coordinates; 0: results only */
  int32_t reserved;
  double lambda0;            /* initial per-landmark damping, default 1e-3 */
  double gradient_tolerance; /* default 1e-6: converged when max_i |b_i| / sqrt(V_ii E) falls to it (MINPACK's gtol) */
  double step_tolerance;     /* default 1e-12: converged when an accepted |delta| <= tol (|x| + tol); 0 = off */
  double min_parallax;       /* rad, default 0 = report only */
  double huber_width;        /* pixels, 0 (default) = plain weighted least squares */
} ba_hip_triangulation_options;
typedef struct {
  uint32_t count[6];         /* landmarks of the last call per status BA_HIP_TRI_* */
  uint32_t landmarks;        /* landmarks requested */
  uint32_t waves;            /* wavefronts launched */
  uint32_t waves_early;      /* ... that held no requested landmark and left after reading the selection */
  uint32_t written;          /* landmarks whose coordinates were replaced */
  double device_ms;          /* event-timed: selection upload to the last kernel */
} ba_hip_triangulation_stats;
/* lm_ids: n landmark ids, each once; NULL: every landmark, n must be the landmark count.  o: NULL = the defaults above.
 * result8 (n x 8, may be NULL), per requested landmark: status, observations used, iterations, cost at the starting
 * point, cost at the end, parallax (rad; the largest angle between the first bearing and any other, the first being
 * the reference ray with LmSize 1), smallest depth over the observing sensors, gradient measure c at the end.
 * x_w4 (n x 4, may be NULL): the world coordinates the call arrived at where it accepts them (whether or not
 * write_back stores them), the coordinates held elsewhere. */
int ba_hip_triangulate_landmarks(ba_hip_engine* e, uint32_t n, const uint32_t* lm_ids, const ba_hip_triangulation_options* o,
                                 double* result8, double* x_w4);
int ba_hip_get_triangulation_stats(ba_hip_engine* e, ba_hip_triangulation_stats* out);

/* ---- Pose refinement (resection), landmarks held fixed (ba_amd/csrc/resect.h) -----------------------
 * The mirror image of ba_hip_triangulate_landmarks: with the landmarks fixed every pose is a 6-parameter least-squares
 * problem of its own over EVERY projection residual it measures, E_p = sum w |z - pi(T_sw X)|^2 with X the landmark's
 * world point.  One launch (k_resect.hip, one workgroup per requested pose) refines each requested pose by
 * Levenberg-Marquardt to convergence, with the cameras of the rig (pinhole and FOV), the per-pose intrinsics when set
 * and the original weights of the observations.  Unary, binary and inertial residuals and dense priors of the pose are
 * NOT part of the cost; the active flags of poses and landmarks are not consulted: the id list decides.  With LmSize 1
 * an observation taken from the landmark's own reference pose counts like any other.  An observation at depth <= 0 (or
 * with a non-finite point) at the starting pose is excluded for the whole call and counted.
 * Uses: a new frame of a window gets its pose from the map (motion-only BA); with write_back = 0 an audit of a
 * trajectory pose by pose (cost, cheirality, and in info36 how well the map determines each pose) that changes nothing.
 * Placement: after ba_hip_finalize, outside a Solve.  Refused with LmSize 0, with calibration unknowns, on a sharded or
 * hooked engine and between ba_hip_begin_solve and ba_hip_end_solve.
 * With write_back the accepted poses replace parameters 0..6 (t, q) of the poses held; velocities, biases and every
 * other pose keep their bits; x_s is re-derived (LmSize 1; the world points stay) and the call then counts as a
 * ba_hip_begin_solve for everything the device holds.  With write_back = 0 nothing the engine holds changes.  Two
 * identical calls return identical bits.  The work space (with the per-pose observation list, built by the first call
 * after a ba_hip_finalize) is allocated by the first call and freed by ba_hip_release_marginals. */
enum {
  BA_HIP_RESECT_OK = 0,                    /* converged; written back */
  BA_HIP_RESECT_NOT_CONVERGED = 1,         /* iteration limit reached; written back if the cost fell */
  BA_HIP_RESECT_TOO_FEW_OBSERVATIONS = 2,  /* 2 x used observations < free parameters; not written */
  BA_HIP_RESECT_FAILED = 3                 /* non-finite starting pose or cost; not written */
};
typedef struct {
  int32_t max_iterations;    /* refinement steps per pose, 0..64; default 20 */
  int32_t write_back;        /* 1 (default): accepted poses replace the poses held; 0: results only */
  uint32_t fixed_mask;       /* bit i (0..5): parameter i (t xyz, rotation xyz) stays; default 0; 63 is refused */
  int32_t reserved;
  double initial_damping;    /* initial per-pose lambda, default 1e-3 */
  double gradient_tolerance; /* default 1e-6: converged when max_i |g_i| / sqrt(H_ii E) falls to it */
                             /* (always: converged when E <= F = sum w (8 eps)^2 |z|^2, the rounding floor of the cost) */
  double step_tolerance;     /* default 1e-12: an accepted |dt| <= tol (|t| + tol) and |dw| <= tol; 0 = off */
  double huber_width;        /* pixels, 0 (default) = plain weighted least squares */
} ba_hip_pose_refinement_options;
typedef struct {
  uint32_t count[4];         /* poses of the last call per status BA_HIP_RESECT_* */
  uint32_t poses;            /* poses requested */
  uint32_t written;          /* poses whose parameters were replaced */
  uint64_t observations_used, observations_excluded;
  double device_ms;          /* event-timed: request upload to the last kernel */
} ba_hip_pose_refinement_stats;
/* pose_ids: n pose ids, each once; NULL: every pose, n must be the pose count.  o: NULL = the defaults above.
 * result8 (n x 8, may be NULL), per requested pose: status, observations used, iterations, cost at the starting pose,
 * cost at the end, smallest depth of a used observation at the end, gradient measure c at the end, observations excluded.
 * t_wp7 (n x 7, may be NULL): t, q (xyzw) of the pose the call arrived at where it accepts it (whether or not write_back
 * stores it), the pose held elsewhere.
 * info36 (n x 36, may be NULL): the undamped H = sum w Jm^T Jm at the end point, full symmetric, row-major, in the
 * engine's parameter order, fixed rows and columns zero (all zero where the refinement did not run).  Scaled by the
 * pixel variance it is the inverse of the localisation covariance. */
int ba_hip_refine_poses(ba_hip_engine* e, uint32_t n, const uint32_t* pose_ids, const ba_hip_pose_refinement_options* o,
                        double* result8, double* t_wp7, double* info36);
int ba_hip_get_pose_refinement_stats(ba_hip_engine* e, ba_hip_pose_refinement_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* BA_HIP_H */
