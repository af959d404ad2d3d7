// Minimal C++ application against include/ba/BundleAdjuster.h — the way the reference's
// applications use the class (cf. /root/reference/applications/unary_binary_imu_test/
// main.cpp:31,60-230: Init / AddPose / Add*Constraint / AddImuResidual / Solve / GetPose).
// Builds a small ring of cameras looking at random points, perturbs the state and runs
// Solve() on the MI355X engine.  Exit code 0 iff the reprojection error went down.
//
//   visual_ba_demo                          ba::BundleAdjuster<double, 1, 6, 0>        (VisualBundleAdjuster)
//   visual_ba_demo --calibrate-intrinsics   ba::BundleAdjuster<double, 1, 6, 4, false> starting from pinhole
//                                           parameters that are 2-3 % off; a third of the poses held fixed
//   visual_ba_demo --calibrate-extrinsics   ba::BundleAdjuster<double, 1, 6, 0, true>  starting from a camera
//                                           mount T_vs that is a few centimetres / half a degree off
//   visual_ba_demo --calibrate-fov          ba::SelfCalBundleAdjuster<double> = <double, 1, 6, 5> (reference
//                                           BundleAdjuster.h:758-759) on a ba::FovCamera whose five parameters
//                                           (fx, fy, u0, v0, w) start 2-4 % off
//   visual_ba_demo --ranks N --rank R --comm-id-file F [--device D]
//                                           one process per GPU: every process holds all poses and the landmarks
//                                           l with l mod N == R; the class joins the engine-owned RCCL communicator
//                                           (SetCommunicator; rank 0 writes the 128-byte id to F, the others wait for
//                                           it) and the reduced solve is distributed over the GPUs — no torch, no hooks
//   visual_ba_demo --ordering auto          Options::pose_ordering = Auto: prints the ordering statistics
//   visual_ba_demo --pcg [tol]              Options::reduced_solver = Pcg (relative tolerance tol, default 1e-6): the reduced
//                                           system is solved by preconditioned conjugate gradients; prints the
//                                           iterations and the true residual of every Gauss-Newton step
//   visual_ba_demo --pcg [tol] --pcg-coarse G   ... with the two-level preconditioner over aggregates of G poses
//                                           (Options::pcg_coarse_aggregate); prints the coarse space of every step
//   visual_ba_demo --pcg [tol] --joint-cov A,B   after the solve: the joint covariance of the poses A and B without a
//                                           factor (GetJointPoseCovarianceIterative: the panel PCG on the twelve unit
//                                           columns), printed as a 12 x 12 block with the passes and the time
//   visual_ba_demo --lm [lambda0]           Options::use_levenberg_marquardt (initial damping lambda0, default 1e-4): damped
//                                           steps accepted by gain ratio; prints lambda and rho of every iteration
//   visual_ba_demo --triangulate [iters]    the landmarks start as directions only (w = 0: the bearing of the reference
//                                           pixel, no depth; with LmSize 3 a point at a fixed wrong range), are
//                                           triangulated and refined with the poses held fixed (TriangulateLandmarks,
//                                           at most iters steps per landmark, default 20), the counts per status are
//                                           printed, then the solve runs as usual
//   visual_ba_demo --refine-poses [iters]   the free poses start 0.3 m off (ten times the plain demo) and are resected
//                                           against the map with the landmarks held fixed (RefinePoses, at most iters
//                                           steps per pose, default 20; 0 = the same start without the refinement), the
//                                           counts per status and the projection cost before and after are printed,
//                                           then the solve runs as usual; composes with --triangulate
//   visual_ba_demo --covariances            after the solve: the last pose's covariance (translation and rotation
//                                           sigmas) and the median landmark sigma (GetPoseCovariance,
//                                           GetLandmarkCovariance: selected inverse of the reduced system), then
//                                           the norm of the cross covariance between the first active and the last
//                                           pose and the time of the joint call (GetJointPoseCovariance), and the
//                                           largest correlation between the last pose and the last landmark with
//                                           the time of that call (GetJointCovariance: the cross blocks)
//   visual_ba_demo --weakest-modes K        after the solve: the K eigenvalues of smallest magnitude of the reduced
//                                           system (GetWeakestModes: block inverse iteration on the kept factor)
//                                           and, per mode, the poses and parameters that carry its largest entries
//   visual_ba_demo --leverages              after the solve: the median and the smallest redundancy number
//                                           2 - tr H_aa of the projection residuals (GetProjectionLeverages: hat
//                                           blocks from the selected inverse) and the five residuals with the
//                                           largest studentised value r^T (I - H_aa)^-1 r, r the whitened residual
#include <ba/BundleAdjuster.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <thread>

struct Shard { int rank = 0, ranks = 1, device = 0; std::string id_file; bool order_auto = false, covariances = false, leverages = false, pcg = false, lm = false; double pcg_tol = 1e-6, lm_lambda0 = 1e-4; unsigned pcg_coarse = 0, weakest_modes = 0; int joint_a = -1, joint_b = -1, triangulate = -1, refine_poses = -1; };

// rank 0 creates the communicator id and publishes it through a file; the other ranks wait for it
static bool exchange_id(const Shard& sh, unsigned char* id) {
  if (sh.rank == 0) {
    if (!ba::BundleAdjuster<double, 1, 6, 0>::CreateCommunicatorId(id)) return false;
    const std::string tmp = sh.id_file + ".tmp";
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f || std::fwrite(id, 1, 128, f) != 128) return false;
    std::fclose(f);
    return std::rename(tmp.c_str(), sh.id_file.c_str()) == 0;
  }
  for (int tries = 0; tries < 600; ++tries) {
    if (FILE* f = std::fopen(sh.id_file.c_str(), "rb")) {
      const size_t n = std::fread(id, 1, 128, f);
      std::fclose(f);
      if (n == 128) return true;
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(100));
  }
  return false;
}

template <class BA>
int run(int calibrate, const Shard& shard = Shard()) {  // 0 none, 1 intrinsics, 2 extrinsics, 3 the five parameters of a FOV camera
  BA adjuster;
  ba::Options<double> options;  // reference defaults: dogleg, robust norm, auto regularisation
  options.error_change_threshold = 1e-5;
  options.device = shard.device;
  if (shard.order_auto) options.pose_ordering = ba::PoseOrdering::Auto;
  if (shard.lm) { options.use_levenberg_marquardt = true; options.use_dogleg = false; options.lm_initial_damping = shard.lm_lambda0; }
  auto print_lm = [&](int step) {
    std::printf("step %d: lambda %.3e rho %.4f rejected %u proj error %.4f\n", step, adjuster.damping(), adjuster.last_gain_ratio(),
                adjuster.rejected_steps(), adjuster.GetSolutionSummary().post_solve_norm);
  };
  if (shard.pcg) { options.reduced_solver = ba::ReducedSolver::Pcg; options.pcg_tolerance = shard.pcg_tol; options.pcg_coarse_aggregate = shard.pcg_coarse; }
  auto print_pcg = [&](int step) {
    ba_hip_pcg_stats ps;
    if (!adjuster.GetPcgStats(&ps)) return;
    std::printf("step %d: pcg iterations %u converged %u true residual %.3e (%.3f ms, %.1f us per product)\n", step, ps.iterations,
                ps.converged, ps.rel_residual_true, ps.solve_ms, 1e3 * ps.spmv_ms);
    ba_hip_pcg_coarse_stats cs;
    if (adjuster.GetPcgCoarseStats(&cs))
      std::printf("step %d: pcg coarse space %u unknowns, %u aggregates of %u (setup %.3f ms, %.1f us per pass)\n", step,
                  cs.coarse_unknowns, cs.aggregates, cs.aggregate_used, cs.setup_ms, 1e3 * cs.apply_ms);
  };
  if (!shard.id_file.empty()) {
    unsigned char id[128];
    if (!exchange_id(shard, id)) { std::printf("communicator id exchange failed\n"); return 3; }
    adjuster.SetCommunicator(id, shard.rank, shard.ranks);
  }
  const int kPoses = 24, kLandmarks = 300;
  adjuster.Init(options, kPoses, kLandmarks * 6, kLandmarks);
  const double fx = 198.969, fy = 198.1284, u0 = 329.9368, v0 = 240.1017, fov_w = 0.93;
  ba::SE3 mount0;  // the true mount is the identity
  if (calibrate == 2) {
    const double t[3] = {0.03, -0.02, 0.02}, q[4] = {0.004, -0.005, 0.003, 1.0};
    mount0 = ba::SE3(t, q);
  }
  const ba::FovCamera<double> true_fov(fx, fy, u0, v0, fov_w);
  if (calibrate == 3)
    adjuster.AddCamera(std::make_shared<ba::FovCamera<double>>(fx * 1.03, fy * 0.97, u0 * 1.02, v0 * 0.98, fov_w * 1.04, mount0));
  else if (calibrate == 1)
    adjuster.AddCamera(std::make_shared<ba::CameraInterface<double>>(fx * 1.03, fy * 0.97, u0 * 1.02, v0 * 0.98, mount0));
  else
    adjuster.AddCamera(std::make_shared<ba::CameraInterface<double>>(fx, fy, u0, v0, mount0));

  std::mt19937 rng(7);
  std::normal_distribution<double> n01(0.0, 1.0);
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  // cameras on a circle of radius 6 looking at the origin
  std::vector<ba::SE3> gt(kPoses);
  for (int i = 0; i < kPoses; ++i) {
    const double a = 2 * M_PI * i / kPoses;
    const double c[3] = {6 * std::cos(a), 6 * std::sin(a), 0.3 * std::sin(3 * a)};
    // z axis -> a target near the origin that wanders with the pose (cameras that all look at ONE
    // point make a shift of the mount along the optical axis a pure change of scale), y axis ~ world -z
    const double tgt[3] = {0.8 * std::sin(2 * a), 0.8 * std::cos(3 * a), 0.2 * std::sin(a)};
    double z[3] = {tgt[0] - c[0], tgt[1] - c[1], tgt[2] - c[2]};
    const double zn = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
    for (double& v : z) v /= zn;
    double x[3] = {z[1], -z[0], 0.0};  // z cross (0,0,1)... any unit vector orthogonal to z
    const double xn = std::sqrt(x[0] * x[0] + x[1] * x[1]);
    for (double& v : x) v /= xn;
    double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    {  // roll about the optical axis
      const double r = 0.5 * std::sin(5 * a), cr = std::cos(r), sr = std::sin(r);
      for (int k = 0; k < 3; ++k) {
        const double xk = cr * x[k] + sr * y[k], yk = -sr * x[k] + cr * y[k];
        x[k] = xk; y[k] = yk;
      }
    }
    const double R[9] = {x[0], y[0], z[0], x[1], y[1], z[1], x[2], y[2], z[2]};
    // rotation matrix -> quaternion (trace branch is fine for this geometry after a sign fix)
    double q[4];
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
      const double s = std::sqrt(tr + 1.0) * 2;
      q[3] = 0.25 * s; q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
      const double s = std::sqrt(1.0 + R[0] - R[4] - R[8]) * 2;
      q[3] = (R[7] - R[5]) / s; q[0] = 0.25 * s; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
      const double s = std::sqrt(1.0 + R[4] - R[0] - R[8]) * 2;
      q[3] = (R[2] - R[6]) / s; q[0] = (R[1] + R[3]) / s; q[1] = 0.25 * s; q[2] = (R[5] + R[7]) / s;
    } else {
      const double s = std::sqrt(1.0 + R[8] - R[0] - R[4]) * 2;
      q[3] = (R[3] - R[1]) / s; q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = 0.25 * s;
    }
    gt[i] = ba::SE3(c, q);
  }
  auto project = [&](const ba::SE3& T, const double* X, double* uv) {
    const ba::Matrix3t R = T.rotationMatrix();
    double d[3] = {X[0] - T.t[0], X[1] - T.t[1], X[2] - T.t[2]}, p[3];
    for (int r = 0; r < 3; ++r) p[r] = R(0, r) * d[0] + R(1, r) * d[1] + R(2, r) * d[2];  // R^T d
    uv[0] = fx * p[0] / p[2] + u0; uv[1] = fy * p[1] / p[2] + v0;
    if (calibrate == 3) {  // the scene is seen through the FOV camera
      const ba::Vector2t d = true_fov.Project(ba::Vector3t({p[0], p[1], p[2]}));
      uv[0] = d[0]; uv[1] = d[1];
    }
    return p[2] > 0.5 && uv[0] > 0 && uv[0] < 640 && uv[1] > 0 && uv[1] < 480;
  };
  for (int i = 0; i < kPoses; ++i) {
    ba::SE3 init = gt[i];
    for (int k = 0; k < 3; ++k) init.t[k] += (shard.refine_poses >= 0 ? 0.3 : 0.03) * n01(rng);
    // two fixed poses pin the gauge (and the scale); self-calibration needs more of them
    const bool fixed = calibrate ? (i % 3 == 0) : (i < 2);
    adjuster.AddPose(fixed ? gt[i] : init, /*is_active=*/!fixed);
  }
  int n_res = 0;
  for (int l = 0; l < kLandmarks; ++l) {
    const double X[3] = {2.5 * (u01(rng) - 0.5), 2.5 * (u01(rng) - 0.5), 1.5 * (u01(rng) - 0.5)};
    int ref = -1;
    double uv[2];
    for (int i = 0; i < kPoses && ref < 0; ++i)
      if (project(gt[(i + l) % kPoses], X, uv)) ref = (i + l) % kPoses;
    if (ref < 0) continue;
    double Xp[4] = {X[0] * (1 + 0.02 * n01(rng)), X[1] * (1 + 0.02 * n01(rng)), X[2], 1.0};
    if (calibrate == 2) {
      // a front end hands over world points built with ITS mount guess: keep the point's coordinates in
      // the reference camera and map them back through T_wp T_vs(guess)
      auto apply = [](const ba::SE3& T, const double* p, double* o) {
        const ba::Matrix3t R = T.rotationMatrix();
        for (int r = 0; r < 3; ++r) o[r] = R(r, 0) * p[0] + R(r, 1) * p[1] + R(r, 2) * p[2] + T.t[r];
      };
      double xs[3], xw[3];
      apply(gt[ref].inverse(), Xp, xs);
      apply(gt[ref] * mount0, xs, xw);
      for (int k = 0; k < 3; ++k) Xp[k] = xw[k];
    }
    if (shard.triangulate >= 0) {
      // no depth: the bearing from the reference pose's centre (LmSize 1: a pure direction), or 5 units along it
      double d[3] = {Xp[0] - gt[ref].t[0], Xp[1] - gt[ref].t[1], Xp[2] - gt[ref].t[2]};
      const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      for (int k = 0; k < 3; ++k) Xp[k] = BA::kLmDim == 1 ? d[k] / len : gt[ref].t[k] + 5.0 * d[k] / len;
      Xp[3] = BA::kLmDim == 1 ? 0.0 : 1.0;
    }
    // landmark shards: every rank draws the same scene, a rank keeps the landmarks l with l mod ranks == rank
    const bool mine = (l % shard.ranks) == shard.rank;
    const uint32_t lm = mine ? adjuster.AddLandmark(ba::Vector4t({Xp[0], Xp[1], Xp[2], Xp[3]}), ref, 0, true) : 0;
    for (int i = 0; i < kPoses; ++i) {
      if (!project(gt[i], X, uv)) continue;
      const ba::Vector2t z({uv[0] + 0.5 * n01(rng), uv[1] + 0.5 * n01(rng)});
      if (mine && adjuster.AddProjectionResidual(z, i, lm, 0) != (uint32_t)-1) ++n_res;
    }
  }
  std::printf("poses %u landmarks %u residuals %d\n", adjuster.GetNumPoses(), adjuster.GetNumLandmarks(), n_res);
  if (shard.triangulate >= 0) {
    ba::TriangulationOptions to;
    to.max_iterations = shard.triangulate;
    std::vector<ba::TriangulationResult> tr;
    if (!adjuster.TriangulateLandmarks({}, to, &tr)) { std::printf("triangulation refused\n"); return 2; }
    unsigned count[6] = {0, 0, 0, 0, 0, 0};
    for (const ba::TriangulationResult& r : tr) count[r.status >= 0 && r.status < 6 ? r.status : 5]++;
    std::printf("triangulated %zu landmarks: ok %u, not converged %u, too few views %u, low parallax %u, behind a camera %u, failed %u\n",
                tr.size(), count[0], count[1], count[2], count[3], count[4], count[5]);
  }
  if (shard.refine_poses >= 0) {
    // the free poses start 0.3 m off (ten times the plain demo): resected against the map, the landmarks held fixed
    ba::PoseRefinementOptions po;
    po.max_iterations = shard.refine_poses;
    std::vector<uint32_t> ids;
    for (int i = 2; i < kPoses; ++i) ids.push_back((uint32_t)i);
    std::vector<ba::PoseRefinementResult> pr;
    if (!adjuster.RefinePoses(ids, po, &pr)) { std::printf("pose refinement refused\n"); return 2; }
    unsigned count[4] = {0, 0, 0, 0};
    double before = 0.0, after = 0.0;
    for (const ba::PoseRefinementResult& r : pr) {
      count[r.status >= 0 && r.status < 4 ? r.status : 3]++;
      before += r.cost_start; after += r.cost_end;
    }
    std::printf("refined %zu poses (%d iterations at most): ok %u, not converged %u, too few observations %u, failed %u; "
                "projection cost of these poses %.6g -> %.6g\n", pr.size(), shard.refine_poses, count[0], count[1], count[2],
                count[3], before, after);
  }
  adjuster.Solve(1);
  if (shard.pcg) print_pcg(1);
  if (shard.lm) print_lm(1);
  if (shard.order_auto) {
    ba_hip_ordering_stats os;
    if (ba_hip_get_pose_ordering(adjuster.engine(), nullptr, &os) != 0) { std::printf("no pose ordering\n"); return 2; }
    std::printf("pose ordering: mode %d candidate %d group %u groups %u tile products %llu -> %llu (%.2f ms host, %.2f ms device)\n",
                os.mode, os.candidate, os.group_size, os.num_groups, (unsigned long long)os.tile_products_natural,
                (unsigned long long)os.tile_products_chosen, os.host_ms, os.device_ms);
  }
  if (!shard.id_file.empty())
    std::printf("rank %d of %d on device %d: reduced solve %s\n", shard.rank, shard.ranks, shard.device,
                adjuster.SolveIsDistributed() ? "distributed over the communicator" : "replicated");
  double e0, eu, eb, ei;
  adjuster.GetErrors(e0, eu, eb, ei);
  if (!adjuster.GetSolutionSummary().IsResultGood()) { std::printf("Solve failed\n"); return 2; }
  if (shard.pcg || shard.lm) {  // one step per call, to print the solver's statistics of each
    for (int it = 0; it < 8; ++it) {
      adjuster.Solve(1);
      if (shard.pcg) print_pcg(it + 2);
      if (shard.lm) print_lm(it + 2);
      if (adjuster.GetSolutionSummary().result != ba::Success) break;
    }
  } else {
    adjuster.Solve(8);
  }
  double e1;
  adjuster.GetErrors(e1, eu, eb, ei);
  double worst = 0;
  for (int i = 0; i < kPoses; ++i) {
    const auto& p = adjuster.GetPose(i);
    for (int k = 0; k < 3; ++k) worst = std::fmax(worst, std::fabs(p.t_wp.t[k] - gt[i].t[k]));
  }
  std::printf("proj error after 1 iteration %.4f, after 9 %.4f, result %d, worst position error %.4f m\n", e0, e1,
              (int)adjuster.GetSolutionSummary().result, worst);
  bool ok = e1 <= e0 && worst < 0.15;
  if (calibrate == 1) {
    const ba::Vector4t p = adjuster.rig()->cameras_[0]->GetParams();
    std::printf("camera parameters %.3f %.3f %.3f %.3f (true %.3f %.3f %.3f %.3f)\n", p[0], p[1], p[2], p[3], fx, fy, u0, v0);
    ok = ok && std::fabs(p[0] - fx) < 0.01 * fx && std::fabs(p[1] - fy) < 0.01 * fy && std::fabs(p[2] - u0) < 0.01 * u0 &&
         std::fabs(p[3] - v0) < 0.01 * v0;
  }
  if (calibrate == 3) {
    const std::vector<double> p = adjuster.rig()->cameras_[0]->ParamsVector();
    std::printf("camera parameters %.3f %.3f %.3f %.3f %.4f (true %.3f %.3f %.3f %.3f %.4f)\n", p[0], p[1], p[2], p[3], p[4],
                fx, fy, u0, v0, fov_w);
    ok = ok && p.size() == 5 && std::fabs(p[0] - fx) < 0.01 * fx && std::fabs(p[1] - fy) < 0.01 * fy &&
         std::fabs(p[2] - u0) < 0.01 * u0 && std::fabs(p[3] - v0) < 0.01 * v0 && std::fabs(p[4] - fov_w) < 0.01 * fov_w;
  }
  if (calibrate == 2) {
    const ba::SE3 m = adjuster.rig()->cameras_[0]->Pose();
    std::printf("camera mount t = %.4f %.4f %.4f  q = %.5f %.5f %.5f %.5f (true: identity)\n", m.t[0], m.t[1], m.t[2], m.q[0],
                m.q[1], m.q[2], m.q[3]);
    const double before = std::sqrt(0.03 * 0.03 + 0.02 * 0.02 + 0.02 * 0.02);
    ok = ok && std::sqrt(m.t[0] * m.t[0] + m.t[1] * m.t[1] + m.t[2] * m.t[2]) < before;
  }
  if (shard.covariances) {
    const ba::MatX c = adjuster.GetPoseCovariance(kPoses - 1);
    std::vector<double> sl;
    for (uint32_t l = 0; l < adjuster.GetNumLandmarks(); ++l) {
      const ba::MatX v = adjuster.GetLandmarkCovariance(l);
      if (v.rows() == 1) sl.push_back(std::sqrt(v(0, 0)));
    }
    if (c.rows() != 6 || sl.empty()) { std::printf("covariances unavailable\n"); return 2; }
    std::nth_element(sl.begin(), sl.begin() + sl.size() / 2, sl.end());
    std::printf("pose %d sigma translation %.3e %.3e %.3e  rotation %.3e %.3e %.3e\n", kPoses - 1, std::sqrt(c(0, 0)),
                std::sqrt(c(1, 1)), std::sqrt(c(2, 2)), std::sqrt(c(3, 3)), std::sqrt(c(4, 4)), std::sqrt(c(5, 5)));
    std::printf("median landmark sigma (inverse depth) %.3e over %zu landmarks\n", sl[sl.size() / 2], sl.size());
    // poses 0 and 1 are fixed: pose 2 is the first with columns in S
    ba::MatX joint;
    const auto j0 = std::chrono::steady_clock::now();
    const bool jok = adjuster.GetJointPoseCovariance({2u, (uint32_t)(kPoses - 1)}, joint);
    const double joint_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - j0).count();
    if (!jok || joint.rows() != 12) { std::printf("joint covariance unavailable\n"); return 2; }
    double cross = 0.0, diag = 0.0;
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) {
        cross += joint(i, 6 + j) * joint(i, 6 + j);
        diag += joint(6 + i, 6 + j) * joint(6 + i, 6 + j);
      }
    std::printf("cross covariance of poses 2 and %d: norm %.3e (%.3e of pose %d's own block), joint call %.3f ms\n", kPoses - 1,
                std::sqrt(cross), std::sqrt(cross / diag), kPoses - 1, joint_ms);
    // the last pose and the last landmark jointly: the pose-landmark cross block
    const uint32_t lm = adjuster.GetNumLandmarks() - 1;
    ba::MatX mixed;
    const auto m0 = std::chrono::steady_clock::now();
    const bool mok = adjuster.GetJointCovariance({(uint32_t)(kPoses - 1)}, {lm}, mixed);
    const double mixed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - m0).count();
    if (!mok || mixed.rows() != 7) { std::printf("joint pose-landmark covariance unavailable\n"); return 2; }
    double corr = 0.0;
    for (int i = 0; i < 6; ++i) corr = std::max(corr, std::fabs(mixed(i, 6)) / std::sqrt(mixed(i, i) * mixed(6, 6)));
    std::printf("pose %d and landmark %u: largest pose-landmark correlation %.3f, joint call %.3f ms\n", kPoses - 1, lm, corr,
                mixed_ms);
    ok = ok && std::isfinite(c(0, 0)) && c(0, 0) > 0 && sl[sl.size() / 2] > 0 && std::isfinite(corr) && corr <= 1.0 + 1e-9;
  }
  if (shard.joint_a >= 0) {
    ba::MatX joint;
    ba_hip_pcg_panel_stats ps;
    if (!adjuster.GetJointPoseCovarianceIterative({(uint32_t)shard.joint_a, (uint32_t)shard.joint_b}, joint, shard.pcg_tol) ||
        joint.rows() != 12 || !adjuster.GetPcgPanelStats(&ps)) {
      std::printf("iterative joint covariance unavailable (it needs --pcg and two different active poses)\n");
      return 2;
    }
    std::printf("joint covariance of poses %d and %d by the panel PCG: %u columns, %u passes, %u converged, largest residual %.2e, "
                "%.3f ms\n", shard.joint_a, shard.joint_b, ps.columns, ps.passes, ps.converged, ps.max_rel_residual_true, ps.solve_ms);
    for (int i = 0; i < 12; ++i) {
      for (int j = 0; j < 12; ++j) std::printf(" % .3e", joint(i, j));
      std::printf("\n");
    }
    for (int i = 0; i < 12; ++i) ok = ok && std::isfinite(joint(i, i)) && joint(i, i) > 0;
    ok = ok && ps.converged == 12;
  }
  if (shard.weakest_modes) {
    std::vector<double> ev;
    ba::MatX modes;
    ba_hip_mode_stats ms;
    if (!adjuster.GetWeakestModes(shard.weakest_modes, ev, modes) || !adjuster.GetModeStats(&ms)) {
      std::printf("weakest modes unavailable\n");
      return 2;
    }
    static const char* names[6] = {"t_x", "t_y", "t_z", "r_x", "r_y", "r_z"};
    const int np = (int)ba_hip_num_pose_params(adjuster.engine());
    std::printf("weakest modes: %u of %zu converged in %u iterations (solve %.3f ms, orthonormalisation %.3f ms)\n", ms.converged,
                ev.size(), ms.iterations, ms.solve_ms, ms.ortho_ms);
    for (size_t i = 0; i < ev.size(); ++i) {
      std::vector<int> idx(modes.cols());
      for (int r = 0; r < modes.cols(); ++r) idx[r] = r;
      const size_t top = std::min<size_t>(3, idx.size());
      std::partial_sort(idx.begin(), idx.begin() + top, idx.end(),
                        [&](int a, int b) { return std::fabs(modes((int)i, a)) > std::fabs(modes((int)i, b)); });
      std::printf("mode %zu: lambda %.6e, largest entries", i, ev[i]);
      for (size_t q = 0; q < top; ++q) {
        const int r = idx[q];
        // poses 0 and 1 are fixed: active pose a is pose a + 2; the rows behind the poses are the calibration's
        if (r < np) std::printf("  pose %d %s %+.3f", r / 6 + 2, names[r % 6], modes((int)i, r));
        else std::printf("  calibration %d %+.3f", r - np, modes((int)i, r));
      }
      std::printf("\n");
      ok = ok && std::isfinite(ev[i]);
    }
  }
  if (shard.leverages) {
    const uint32_t nres = adjuster.GetNumProjResiduals();
    std::vector<double> h, red(nres);
    if (!adjuster.GetProjectionLeverages({}, h) || h.size() != 4 * (size_t)nres) { std::printf("leverages unavailable\n"); return 2; }
    for (uint32_t a = 0; a < nres; ++a) red[a] = 2.0 - (h[4 * (size_t)a] + h[4 * (size_t)a + 3]);
    // studentised residuals on the host: the whitened residual against the post-fit covariance I - H_aa
    std::vector<std::pair<double, uint32_t>> stud(nres);
    for (uint32_t a = 0; a < nres; ++a) {
      const auto& r = adjuster.GetProjectionResidual(a);
      const double sw = std::sqrt(r.weight), r0 = sw * r.residual[0], r1 = sw * r.residual[1];
      const double c00 = 1.0 - h[4 * (size_t)a], c01 = -h[4 * (size_t)a + 1], c11 = 1.0 - h[4 * (size_t)a + 3];
      const double det = c00 * c11 - c01 * c01;
      stud[a] = {det > 1e-12 ? (c11 * r0 * r0 - 2.0 * c01 * r0 * r1 + c00 * r1 * r1) / det : 0.0, a};
    }
    std::vector<double> sorted(red);
    std::nth_element(sorted.begin(), sorted.begin() + sorted.size() / 2, sorted.end());
    std::printf("redundancy of %u projection residuals: median %.4f, minimum %.4f\n", nres, sorted[sorted.size() / 2],
                *std::min_element(red.begin(), red.end()));
    const size_t top = std::min<size_t>(5, stud.size());
    std::partial_sort(stud.begin(), stud.begin() + top, stud.end(), std::greater<std::pair<double, uint32_t>>());
    for (size_t q = 0; q < top; ++q) {
      const auto& r = adjuster.GetProjectionResidual(stud[q].second);
      std::printf("residual %u (pose %u, landmark %u): studentised %.3f, redundancy %.4f\n", stud[q].second, r.x_meas_id,
                  r.landmark_id, stud[q].first, red[stud[q].second]);
    }
    for (double v : red) ok = ok && v > -1e-9 && v < 2.0 + 1e-9;
  }
  return ok ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--calibrate-intrinsics") == 0) return run<ba::BundleAdjuster<double, 1, 6, 4, false>>(1);
  if (argc > 1 && std::strcmp(argv[1], "--calibrate-extrinsics") == 0) return run<ba::BundleAdjuster<double, 1, 6, 0, true>>(2);
  if (argc > 1 && std::strcmp(argv[1], "--calibrate-fov") == 0) return run<ba::SelfCalBundleAdjuster<double>>(3);
  Shard shard;
  for (int i = 1; i < argc; i += 2) {
    if (std::strcmp(argv[i], "--covariances") == 0) { shard.covariances = true; --i; continue; }
    if (std::strcmp(argv[i], "--leverages") == 0) { shard.leverages = true; --i; continue; }
    if (std::strcmp(argv[i], "--lm") == 0) {
      shard.lm = true;
      if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) shard.lm_lambda0 = std::atof(argv[i + 1]);
      else --i;
      continue;
    }
    if (std::strcmp(argv[i], "--triangulate") == 0) {
      shard.triangulate = 20;
      if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) shard.triangulate = std::atoi(argv[i + 1]);
      else --i;
      continue;
    }
    if (std::strcmp(argv[i], "--refine-poses") == 0) {
      shard.refine_poses = 20;
      if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) shard.refine_poses = std::atoi(argv[i + 1]);
      else --i;
      continue;
    }
    if (std::strcmp(argv[i], "--pcg") == 0) {
      shard.pcg = true;
      if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) shard.pcg_tol = std::atof(argv[i + 1]);
      else --i;
      continue;
    }
    if (i + 1 >= argc) break;
    if (std::strcmp(argv[i], "--weakest-modes") == 0) shard.weakest_modes = (unsigned)std::atoi(argv[i + 1]);
    else if (std::strcmp(argv[i], "--pcg-coarse") == 0) shard.pcg_coarse = (unsigned)std::atoi(argv[i + 1]);
    else if (std::strcmp(argv[i], "--joint-cov") == 0) {
      if (std::sscanf(argv[i + 1], "%d,%d", &shard.joint_a, &shard.joint_b) != 2 || shard.joint_a < 0 || shard.joint_b < 0) {
        std::printf("bad --joint-cov (two pose ids: A,B)\n");
        return 3;
      }
    }
    else if (std::strcmp(argv[i], "--ranks") == 0) shard.ranks = std::atoi(argv[i + 1]);
    else if (std::strcmp(argv[i], "--rank") == 0) shard.rank = std::atoi(argv[i + 1]);
    else if (std::strcmp(argv[i], "--device") == 0) shard.device = std::atoi(argv[i + 1]);
    else if (std::strcmp(argv[i], "--comm-id-file") == 0) shard.id_file = argv[i + 1];
    else if (std::strcmp(argv[i], "--ordering") == 0) shard.order_auto = std::strcmp(argv[i + 1], "auto") == 0;
  }
  if (shard.ranks < 1 || shard.rank < 0 || shard.rank >= shard.ranks) { std::printf("bad --rank / --ranks\n"); return 3; }
  return run<ba::BundleAdjuster<double, 1, 6, 0>>(0, shard);  // VisualBundleAdjuster<double>
}
