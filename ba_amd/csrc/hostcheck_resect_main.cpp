// Stand-alone driver of the per-pose observation list and the host restatement of the pose refinement of resect.h
// (through ba_hostcheck_pose_obs_lists and ba_hostcheck_refine_poses of hostcheck.cpp), for a sanitizer build:
//   make -C ba_amd/csrc ../lib/hostcheck_resect_asan && ba_amd/lib/hostcheck_resect_asan
// One synthetic window restated from tests/resection_cases.py: poses on a ring looking at a ball of landmarks, the poses
// measuring 0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1 024, 1 025 and 1 100 landmarks (the edges of the kernel's paths), a
// two-camera rig, true pixels, every pose off by 0.1 m and 3 degrees; then the same with an id list, a fixed_mask, a
// Huber width and a landmark behind a camera, and the refusals.  Every buffer has exactly the size the entry fills.
// Checked here: the return codes, that the list is the stable sort by pose, statuses and counts, and that the poses of
// at least 63 observations come back to 1e-9; the bounds proper are the subject of tests/test_resection.py.
// Prints the totals and "ok".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

extern "C" int ba_hostcheck_pose_obs_lists(uint32_t P, uint32_t O, const uint32_t* obs_pose, uint32_t* ptr, uint32_t* idx);
extern "C" int ba_hostcheck_refine_poses(uint32_t P, const double* poses7, uint32_t C, const double* cam_params4,
                                         const double* cam_tvs7, const int32_t* cam_model, const double* cam_w,
                                         const double* pose_cam4, uint32_t O, const uint32_t* obs_pose,
                                         const uint32_t* obs_cam, const uint32_t* obs_lm, const double* obs_z,
                                         const double* obs_w0, const double* x_w, uint32_t n, const uint32_t* ids,
                                         const double* opts7, double* res, double* t_out, double* info, double* final,
                                         char* msg, uint32_t cap);

static int fail(const char* what) {
  fprintf(stderr, "hostcheck_resect: %s\n", what);
  return 1;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*, in [0, 1)
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

static void quat_to_rot(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
static void quat_mul(const double* a, const double* b, double* o) {
  const double r[4] = {a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                       a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]};
  const double n = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
  for (int i = 0; i < 4; ++i) o[i] = r[i] / n;
}
static void quat_exp(double wx, double wy, double wz, double* q) {
  const double th = sqrt(wx * wx + wy * wy + wz * wz), s = th > 0 ? sin(0.5 * th) / th : 0.5;
  q[0] = s * wx; q[1] = s * wy; q[2] = s * wz; q[3] = cos(0.5 * th);
}

int main() {
  const uint32_t counts[] = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1024, 1025, 1100};
  const uint32_t P = sizeof(counts) / sizeof(counts[0]), C = 2, L = 1141;   // (landmark L - 1 is the one behind a camera)
  const double cam_params[8] = {500, 505, 320, 240, 420, 415, 300, 250};
  double cam_tvs[14] = {0.10, -0.05, 0.02, 0, 0, 0, 1, -0.20, 0.03, 0.05, 0, 0, 0, 1};
  quat_exp(0.05, -0.1, 0.03, cam_tvs + 3);
  quat_exp(-0.04, 0.12, 0.2, cam_tvs + 10);
  // landmarks in a ball of radius 2; poses on a ring of radius 8 looking at its centre (yaw about y, then a roll)
  std::vector<double> x_w((size_t)L * 4), truth((size_t)P * 7), poses((size_t)P * 7);
  for (uint32_t l = 0; l < L; ++l) {
    double v[3], n2;
    do { n2 = 0; for (int i = 0; i < 3; ++i) { v[i] = 2 * uniform() - 1; n2 += v[i] * v[i]; } } while (n2 > 1.0 || n2 < 0.01);
    for (int i = 0; i < 3; ++i) x_w[(size_t)l * 4 + i] = 2.0 * v[i];
    x_w[(size_t)l * 4 + 3] = 1.0;
  }
  for (uint32_t p = 0; p < P; ++p) {
    const double a = 2 * uniform() - 1;
    double* t = &truth[(size_t)p * 7];
    t[0] = 8 * sin(a); t[1] = 0.0; t[2] = -8 * cos(a);
    double yaw[4], roll[4];
    quat_exp(0, -a, 0, yaw);            // the camera's z axis turns from +z to -position
    quat_exp(0, 0, uniform() - 0.5, roll);
    quat_mul(yaw, roll, t + 3);
    double u[3] = {uniform() - 0.5, uniform() - 0.5, uniform() - 0.5}, w[3] = {uniform() - 0.5, uniform() - 0.5, uniform() - 0.5};
    const double un = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), wn = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double* s = &poses[(size_t)p * 7];
    for (int i = 0; i < 3; ++i) s[i] = t[i] + 0.1 * u[i] / un;
    double dq[4];
    const double ang = 3.0 * M_PI / 180.0;
    quat_exp(ang * w[0] / wn, ang * w[1] / wn, ang * w[2] / wn, dq);
    quat_mul(t + 3, dq, s + 3);
  }
  // observations in the caller's order (pose by pose), true pixels through T_sw = (T_wp T_vs)^-1; then sorted by landmark
  struct Ob { uint32_t pose, cam, lm; double z[2], w; };
  std::vector<Ob> obs;
  for (uint32_t p = 0; p < P; ++p)
    for (uint32_t j = 0; j < counts[p]; ++j) {
      Ob o;
      o.pose = p; o.cam = (j + p) % C; o.lm = (j * 7 + p * 13) % (L - 1); o.w = 0.5 + 1.5 * uniform();
      // (j * 7 mod 1140 visits distinct landmarks for j < 1140: each landmark at most once per pose)
      const double* t = &truth[(size_t)p * 7];
      const double* tv = cam_tvs + 7 * o.cam;
      double Rp[9], Rv[9];
      quat_to_rot(t + 3, Rp);
      quat_to_rot(tv + 3, Rv);
      const double* X = &x_w[(size_t)o.lm * 4];
      double d[3] = {X[0] - t[0], X[1] - t[1], X[2] - t[2]}, pp[3], ps[3];
      for (int i = 0; i < 3; ++i) pp[i] = Rp[i] * d[0] + Rp[3 + i] * d[1] + Rp[6 + i] * d[2] - tv[i];
      for (int i = 0; i < 3; ++i) ps[i] = Rv[i] * pp[0] + Rv[3 + i] * pp[1] + Rv[6 + i] * pp[2];
      if (!(ps[2] > 0)) return fail("the window puts a landmark behind a camera");
      const double* k = cam_params + 4 * o.cam;
      o.z[0] = k[0] * ps[0] / ps[2] + k[2]; o.z[1] = k[1] * ps[1] / ps[2] + k[3];
      obs.push_back(o);
    }
  // one more observation of pose 6 (65 -> 66): a map point behind its camera
  {
    const double* t = &truth[6 * 7];
    double R[9];
    quat_to_rot(t + 3, R);
    for (int i = 0; i < 3; ++i) x_w[(size_t)(L - 1) * 4 + i] = t[i] - 2.0 * R[3 * i + 2];
    Ob o = {6, 0, L - 1, {300.0, 200.0}, 1.0};
    obs.push_back(o);
  }
  const uint32_t O = (uint32_t)obs.size();
  std::vector<uint32_t> by_lm(O), lm_count(L + 1, 0);
  for (const Ob& o : obs) lm_count[o.lm + 1] += 1;
  for (uint32_t l = 0; l < L; ++l) lm_count[l + 1] += lm_count[l];
  {
    std::vector<uint32_t> at(lm_count.begin(), lm_count.end() - 1);
    for (uint32_t a = 0; a < O; ++a) by_lm[at[obs[a].lm]++] = a;
  }
  std::vector<uint32_t> obs_pose(O), obs_cam(O), obs_lm(O);
  std::vector<double> obs_z((size_t)O * 2), obs_w(O);
  for (uint32_t s = 0; s < O; ++s) {
    const Ob& o = obs[by_lm[s]];
    obs_pose[s] = o.pose; obs_cam[s] = o.cam; obs_lm[s] = o.lm; obs_z[2 * (size_t)s] = o.z[0]; obs_z[2 * (size_t)s + 1] = o.z[1];
    obs_w[s] = o.w;
  }

  // the list: exact sizes, the stable sort by pose
  std::vector<uint32_t> ptr(P + 1), idx(O);
  if (ba_hostcheck_pose_obs_lists(P, O, obs_pose.data(), ptr.data(), idx.data()) != 0) return fail("list builder refused");
  for (uint32_t p = 0; p < P; ++p) {
    if (ptr[p + 1] - ptr[p] != counts[p] + (p == 6 ? 1 : 0)) return fail("list: count of a pose");
    for (uint32_t j = ptr[p]; j < ptr[p + 1]; ++j) {
      if (obs_pose[idx[j]] != p) return fail("list: entry of another pose");
      if (j > ptr[p] && idx[j] <= idx[j - 1]) return fail("list: entries not ascending");
    }
  }
  {
    std::vector<uint32_t> one_ptr(2), none_ptr(4), bad_ptr(3), bad_idx(2);
    const uint32_t bad_pose[2] = {0, 2};
    if (ba_hostcheck_pose_obs_lists(1, 0, nullptr, one_ptr.data(), nullptr) != 0 || one_ptr[1] != 0) return fail("list: P = 1, O = 0");
    if (ba_hostcheck_pose_obs_lists(3, 0, nullptr, none_ptr.data(), nullptr) != 0) return fail("list: no observations");
    if (ba_hostcheck_pose_obs_lists(2, 2, bad_pose, bad_ptr.data(), bad_idx.data()) != 1) return fail("list: a pose out of range passed");
  }

  // the restatement: every pose at the defaults
  char msg[256];
  unsigned long iterations = 0, used = 0, excluded = 0, refusals = 0;
  const double defaults[7] = {20, 1, 0, 1e-3, 1e-6, 1e-12, 0};
  auto call = [&](uint32_t n, const uint32_t* ids, const double* opts, std::vector<double>* res, std::vector<double>* t7) {
    res->assign((size_t)n * 8, -1.0);
    t7->assign((size_t)n * 7, 0.0);
    std::vector<double> info((size_t)n * 36), final((size_t)n * 7);
    return ba_hostcheck_refine_poses(P, poses.data(), C, cam_params, cam_tvs, nullptr, nullptr, nullptr, O, obs_pose.data(),
                                     obs_cam.data(), obs_lm.data(), obs_z.data(), obs_w.data(), x_w.data(), n, ids, opts,
                                     res->data(), t7->data(), info.data(), final.data(), msg, sizeof(msg));
  };
  std::vector<double> res, t7;
  if (call(P, nullptr, defaults, &res, &t7) != 0) return fail(msg);
  for (uint32_t p = 0; p < P; ++p) {
    const double* r = &res[(size_t)p * 8];
    const int want = counts[p] < 3 ? 2 : -1;
    if (want >= 0 && (int)r[0] != want) return fail("status of a pose below 3 observations");
    if (want < 0 && (int)r[0] > 1) return fail("status of a refined pose");
    if ((uint32_t)r[1] != counts[p] || (uint32_t)r[7] != (p == 6 ? 1u : 0u)) return fail("used / excluded counts");
    iterations += (unsigned long)r[2]; used += (unsigned long)r[1]; excluded += (unsigned long)r[7];
    for (int i = 0; i < 7; ++i) {
      const double got = t7[(size_t)p * 7 + i];
      if (counts[p] < 3 && memcmp(&got, &poses[(size_t)p * 7 + i], sizeof(double)) != 0) return fail("an unrefined pose changed");
      const double sign = t7[(size_t)p * 7 + 6] * truth[(size_t)p * 7 + 6] < 0 && i >= 3 ? -1.0 : 1.0;
      if (counts[p] >= 63 && fabs(got - sign * truth[(size_t)p * 7 + i]) > 1e-9) return fail("a pose did not come back to the truth");
    }
  }
  // an id list with a fixed_mask and a Huber width; max_iterations 0 and 64
  {
    const uint32_t ids[5] = {12, 0, 6, 3, 9};
    const double masked[7] = {64, 0, 7, 1e-3, 1e-6, 1e-12, 2.0}, none[7] = {0, 1, 56, 0.0, 0.0, 0.0, 0.0};
    if (call(5, ids, masked, &res, &t7) != 0) return fail(msg);
    for (uint32_t i = 0; i < 5; ++i)
      if (memcmp(&t7[(size_t)i * 7], &poses[(size_t)ids[i] * 7], 3 * sizeof(double)) != 0) return fail("fixed translation moved");
    if ((int)res[3 * 8] > 1) return fail("3 observations serve 3 free parameters");
    if (call(5, ids, none, &res, &t7) != 0) return fail(msg);
    for (uint32_t i = 0; i < 5; ++i)
      if (res[(size_t)i * 8 + 2] != 0.0) return fail("max_iterations 0 iterated");
    if (call(1, ids + 1, defaults, &res, &t7) != 0 || (int)res[0] != 2) return fail("a pose without observations");
  }
  // a NaN pixel on poses 3 (3 observations) and 9 (257): FAILED exactly, pose bit for bit, zero cost and information;
  // a NaN pose 7: TOO_FEW_OBSERVATIONS with every observation excluded; pose 8 beside them as before
  {
    const std::vector<double> z_saved = obs_z, poses_saved = poses;
    unsigned spoilt = 0;
    for (uint32_t s = 0; s < O && spoilt != 3; ++s) {
      if (obs_pose[s] == 3 && !(spoilt & 1)) { obs_z[2 * (size_t)s + 1] = NAN; spoilt |= 1; }
      if (obs_pose[s] == 9 && !(spoilt & 2)) { obs_z[2 * (size_t)s] = NAN; spoilt |= 2; }
    }
    poses[7 * 7 + 1] = NAN;
    const uint32_t ids[4] = {3, 9, 7, 8};
    if (call(4, ids, defaults, &res, &t7) != 0) return fail(msg);
    if ((int)res[0] != 3 || (int)res[8] != 3) return fail("a NaN pixel did not give FAILED");
    if ((uint32_t)res[1] != 3 || (uint32_t)res[8 + 1] != 257 || res[2] != 0 || res[3] != 0 || res[4] != 0 || res[8 + 4] != 0)
      return fail("the row of a FAILED pose");
    if ((int)res[16] != 2 || res[16 + 1] != 0 || (uint32_t)res[16 + 7] != 255) return fail("a NaN pose is TOO_FEW_OBSERVATIONS");
    if ((int)res[24] != 0) return fail("the neighbour of a FAILED pose");
    for (uint32_t i = 0; i < 3; ++i)
      if (memcmp(&t7[(size_t)i * 7], &poses[(size_t)ids[i] * 7], 7 * sizeof(double)) != 0) return fail("a FAILED pose changed");
    obs_z = z_saved;
    poses = poses_saved;
  }
  // refusals
  {
    const uint32_t twice[2] = {1, 1}, far[1] = {P};
    const double mask63[7] = {20, 1, 63, 1e-3, 1e-6, 1e-12, 0}, iters[7] = {65, 1, 0, 1e-3, 1e-6, 1e-12, 0},
                 neg[7] = {20, 1, 0, 1e-3, -1e-6, 1e-12, 0};
    refusals += call(2, twice, defaults, &res, &t7) == 1;
    refusals += call(1, far, defaults, &res, &t7) == 1;
    refusals += call(0, twice, defaults, &res, &t7) == 1;
    refusals += call(P - 1, nullptr, defaults, &res, &t7) == 1;
    refusals += call(P, nullptr, mask63, &res, &t7) == 1;
    refusals += call(P, nullptr, iters, &res, &t7) == 1;
    refusals += call(P, nullptr, neg, &res, &t7) == 1;
    if (refusals != 7) return fail("a bad request was served");
  }
  printf("hostcheck_resect: %u poses, %u observations, %lu used, %lu excluded, %lu iterations, %lu refusals\nok\n", P, O, used,
         excluded, iterations, refusals);
  return 0;
}
