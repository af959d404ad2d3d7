// Stand-alone driver of the two host entry points of the joint state covariances (hostcheck.cpp:
// ba_hostcheck_joint_rhs, ba_hostcheck_joint_state) over random inputs, for a sanitizer build:
//   make -C ba_amd/csrc ../lib/hostcheck_joint_state_asan && ba_amd/lib/hostcheck_joint_state_asan
// LmSize 1 and 3, inactive poses and landmarks, landmarks without observations, duplicate observations, requests
// whose reach is empty.  Checks symmetry and that V^-1 = 1e6 I is read for an unobserved landmark; prints "ok".
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

extern "C" int ba_hostcheck_joint_rhs(uint32_t n, const double* S, uint32_t m, const double* B, double* cov, double* Y_out,
                                      uint8_t* reach_out, uint32_t* level_of, uint8_t* nzL_out, uint64_t* products,
                                      uint32_t* levels);
extern "C" int ba_hostcheck_joint_state(int LM, int D, int K, uint32_t P, const uint8_t* pose_active, uint32_t L,
                                        const uint8_t* lm_active, const uint32_t* lm_ref_pose, uint32_t O,
                                        const uint32_t* proj_pose, const uint32_t* proj_lm, const double* jm12,
                                        const double* jr12, const double* jl, const double* jk12, const double* w,
                                        uint32_t n, const double* S, uint32_t n_poses, const uint32_t* pose_ids,
                                        int include_calibration, uint32_t n_lms, const uint32_t* lm_ids, int variant,
                                        double* cov, uint8_t* reach_out);

static std::mt19937 rng(7);
static double rnd() { return std::normal_distribution<double>()(rng); }

// banded, strictly diagonally dominant
static std::vector<double> random_spd(uint32_t n, uint32_t band) {
  std::vector<double> S((size_t)n * n, 0.0);
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = r + 1; c < std::min(n, r + band); ++c) S[(size_t)r * n + c] = S[(size_t)c * n + r] = rnd();
  for (uint32_t r = 0; r < n; ++r) {
    double s = 1.0;
    for (uint32_t c = 0; c < n; ++c) s += c == r ? 0.0 : std::abs(S[(size_t)r * n + c]);
    S[(size_t)r * n + r] = s;
  }
  return S;
}

static int fail(const char* what) {
  fprintf(stderr, "hostcheck_joint_state: %s\n", what);
  return 1;
}

static int symmetric(const std::vector<double>& cov, uint32_t m) {
  for (uint32_t a = 0; a < m; ++a)
    for (uint32_t b = 0; b < a; ++b)
      if (cov[(size_t)a * m + b] != cov[(size_t)b * m + a]) return 0;
  return 1;
}

static int run_rhs(uint32_t n, uint32_t m, int zero) {
  const uint32_t nt = (n + 63) / 64;
  std::vector<double> S = random_spd(n, 20), B((size_t)n * m, 0.0), cov((size_t)m * m), Y((size_t)64 * nt * m);
  if (!zero)
    for (uint32_t c = 0; c + 1 < m; ++c)   // (the last column stays zero)
      for (int k = 0; k < 5; ++k) B[(size_t)(rng() % n) * m + c] = rnd();
  std::vector<uint8_t> reach(nt), nzL((size_t)nt * nt);
  std::vector<uint32_t> level(nt);
  uint64_t prod;
  uint32_t lev;
  if (ba_hostcheck_joint_rhs(n, S.data(), m, B.data(), cov.data(), Y.data(), reach.data(), level.data(), nzL.data(), &prod, &lev))
    return fail("ba_hostcheck_joint_rhs returned an error");
  if (!symmetric(cov, m)) return fail("joint_rhs: not symmetric");
  if (zero && (prod != 0 || lev != 0)) return fail("joint_rhs: an empty reach was visited");
  return 0;
}

static int run_state(int LM, uint32_t P, uint32_t L, uint32_t per_lm) {
  std::vector<uint8_t> pa(P, 1), la(L, 1);
  for (uint32_t p = 0; p < P; p += 5) pa[p] = 0;
  la[1] = 0;
  std::vector<uint32_t> ref(L), pp, pl;
  for (uint32_t l = 0; l < L; ++l) {
    ref[l] = rng() % P;
    if (l == 2) continue;                     // landmark 2: active, no observation
    for (uint32_t k = 0; k < per_lm; ++k) {
      uint32_t p = (ref[l] + 1 + rng() % 9) % P;
      if (l == 3) p = 0;                      // landmark 3: every observing pose inactive
      pp.push_back(p); pl.push_back(l);
      if (l == 4 && k == 0) { pp.push_back(p); pl.push_back(l); }   // a duplicate
    }
  }
  const uint32_t O = (uint32_t)pp.size();
  std::vector<double> jm((size_t)O * 12), jr((size_t)O * 12), jl((size_t)O * 2 * LM), w(O);
  for (double& x : jm) x = rnd();
  for (double& x : jr) x = rnd();
  for (double& x : jl) x = rnd();
  for (double& x : w) x = 0.5 + (rng() % 100) / 100.0;
  uint32_t nact = 0;
  for (uint8_t a : pa) nact += a;
  const uint32_t n = nact * 6;
  std::vector<double> S = random_spd(n, 30);
  std::vector<uint32_t> poses, lms = {2, 4, 0, 3, L - 1};
  for (uint32_t p = P; p-- > 0 && poses.size() < 3;)
    if (pa[p]) poses.push_back(p);
  std::vector<uint8_t> reach((n + 63) / 64);
  for (int variant = 0; variant < 4; ++variant) {
    const uint32_t M = (uint32_t)poses.size() * 6 + (uint32_t)lms.size() * LM;
    std::vector<double> cov((size_t)M * M);
    if (ba_hostcheck_joint_state(LM, 6, 0, P, pa.data(), L, la.data(), ref.data(), O, pp.data(), pl.data(), jm.data(), jr.data(),
                                 jl.data(), nullptr, w.data(), n, S.data(), (uint32_t)poses.size(), poses.data(), 0,
                                 (uint32_t)lms.size(), lms.data(), variant, cov.data(), reach.data()))
      return fail("ba_hostcheck_joint_state returned an error");
    if (!symmetric(cov, M)) return fail("joint_state: not symmetric");
    const size_t c = poses.size() * 6;   // landmark 2 comes first
    if (variant == 0 && cov[c * M + c] != 1e6) return fail("joint_state: an unobserved landmark does not read 1e6");
  }
  // an empty reach: the unobserved landmark alone; an inactive landmark is refused
  const uint32_t only[1] = {2}, off[1] = {1};
  std::vector<double> cov((size_t)LM * LM);
  if (ba_hostcheck_joint_state(LM, 6, 0, P, pa.data(), L, la.data(), ref.data(), O, pp.data(), pl.data(), jm.data(), jr.data(),
                               jl.data(), nullptr, w.data(), n, S.data(), 0, nullptr, 0, 1, only, 0, cov.data(), reach.data()))
    return fail("joint_state: the empty reach returned an error");
  for (uint8_t r : reach)
    if (r) return fail("joint_state: an empty reach was visited");
  if (ba_hostcheck_joint_state(LM, 6, 0, P, pa.data(), L, la.data(), ref.data(), O, pp.data(), pl.data(), jm.data(), jr.data(),
                               jl.data(), nullptr, w.data(), n, S.data(), 0, nullptr, 0, 1, off, 0, cov.data(), reach.data()) != -3)
    return fail("joint_state: an inactive landmark was served");
  return 0;
}

int main() {
  for (uint32_t n : {43u, 128u, 200u})
    for (uint32_t m : {1u, 9u, 70u})
      if (run_rhs(n, m, 0) || run_rhs(n, m, 1)) return 1;
  for (int LM : {1, 3})
    for (uint32_t P : {12u, 40u})
      if (run_state(LM, P, 3 * P, 4)) return 1;
  printf("ok\n");
  return 0;
}
