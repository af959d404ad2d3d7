// Stand-alone driver of the request layer (requests.h through the taps of hostcheck.cpp: ba_hostcheck_guard,
// ba_hostcheck_selection, ba_hostcheck_request_check, ba_hostcheck_rowmaps), for a sanitizer build:
//   make -C ba_amd/csrc ../lib/hostcheck_requests_asan && ba_amd/lib/hostcheck_requests_asan
// The structure of tests/test_requests.py (5 poses, pose 1 inactive; 4 landmarks, landmark 2 inactive; PoseSize 6 / 15,
// 0 / 6 calibration rows, LmSize 0 / 1 / 3, natural order and the ordering [2, 0, 3, 1]): accepted selections, every
// refusal, requests at and over the column limits, n = 0 with NULL id pointers; every guard after every prefix of a
// direct and a PCG round, under every combination of the engine facts.  Prints the counts and "ok".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "lifecycle.h"

extern "C" int ba_hostcheck_guard(uint32_t n, const int32_t* events, const char* guard, const char* who, const char* noun,
                                  uint32_t facts, uint32_t flags, double rel_tolerance, uint32_t coarse_aggregate, char* msg,
                                  uint32_t cap);
extern "C" int ba_hostcheck_selection(uint32_t P, const int32_t* pose_opt, uint32_t L, const int32_t* lm_opt, uint32_t np,
                                      uint32_t K, uint32_t D, uint32_t LM, uint32_t ld, uint32_t n_perm,
                                      const uint32_t* opt_of_natural, const char* who, uint32_t n_poses, const uint32_t* pose_ids,
                                      int include_calibration, uint32_t n_lms, const uint32_t* lm_ids, int have_out,
                                      uint64_t limit, const char* limit_name, const char* nothing, int caller_numbering,
                                      uint32_t* rows_out, uint32_t* lms_out, uint32_t* counts, char* msg, uint32_t cap);
extern "C" int ba_hostcheck_request_check(int op, const char* who, const char* name, const uint64_t* u, const double* d, char* msg,
                                          uint32_t cap);
extern "C" void ba_hostcheck_rowmaps(uint32_t np, uint32_t K, uint32_t D, uint32_t ld, uint32_t n_perm,
                                     const uint32_t* opt_of_natural, uint32_t* natural_out, uint32_t* identity_out);

static int fail(const char* what) {
  fprintf(stderr, "hostcheck_requests: %s\n", what);
  return 1;
}

static unsigned served = 0, refused = 0;

struct Case {
  uint32_t D, K, LM;
  bool perm;
};

// one request; `want`: a piece of the refusal's message, or null for an accepted one (then the rows are checked)
static int ask(const Case& c, std::vector<uint32_t> poses, std::vector<uint32_t> lms, bool cal, bool caller, const char* want,
               bool null_ids = false) {
  const int32_t nat[5] = {0, -1, 1, 2, 3};
  const uint32_t perm[4] = {2, 0, 3, 1};
  int32_t pose_opt[5], lm_opt[4] = {-1, -1, -1, -1};
  for (int p = 0; p < 5; ++p) pose_opt[p] = nat[p] < 0 ? -1 : c.perm ? (int32_t)perm[nat[p]] : nat[p];
  if (c.LM) { lm_opt[0] = 0; lm_opt[1] = 1; lm_opt[3] = 2; }
  const uint32_t np = 4 * c.D, n = np + c.K, ld = (n + 63) / 64 * 64;
  // exactly as many slots as an accepted request fills: the sanitizer sees one row too many
  std::vector<uint32_t> rows(poses.size() * c.D + (cal ? c.K : 0)), out_lms(lms.size());
  uint32_t counts[2] = {0, 0};
  char msg[256];
  const int rc = ba_hostcheck_selection(
      5, pose_opt, 4, lm_opt, np, c.K, c.D, c.LM, ld, c.perm ? 4 : 0, c.perm ? perm : nullptr, "who", (uint32_t)poses.size(),
      null_ids ? nullptr : poses.data(), cal, (uint32_t)lms.size(), null_ids ? nullptr : lms.data(), 1, 512,
      caller ? "BA_HIP_PCG_PANEL_MAX_COLUMNS" : "BA_HIP_JOINT_MAX_COLUMNS", "nothing requested", caller, rows.data(),
      out_lms.data(), counts, msg, sizeof(msg));
  if (want) {
    if (rc != 1 || !strstr(msg, want)) { fprintf(stderr, "got %d \"%s\", want \"%s\"\n", rc, rc ? msg : "", want); return fail("refusal"); }
    ++refused;
    return 0;
  }
  if (rc != 0 || counts[0] != rows.size() || counts[1] != lms.size()) return fail("an accepted selection was refused");
  std::vector<uint32_t> natural(ld), identity(ld);
  ba_hostcheck_rowmaps(np, c.K, c.D, ld, c.perm ? 4 : 0, c.perm ? perm : nullptr, natural.data(), identity.data());
  size_t k = 0;
  for (uint32_t p : poses)
    for (uint32_t x = 0; x < c.D; ++x, ++k) {
      const uint32_t engine_row = (uint32_t)pose_opt[p] * c.D + x;
      if (rows[k] != (caller ? natural[engine_row] : engine_row)) return fail("a pose row");
    }
  for (uint32_t x = 0; cal && x < c.K; ++x, ++k)
    if (rows[k] != np + x) return fail("a calibration row");
  for (size_t i = 0; i < lms.size(); ++i)
    if (out_lms[i] != lms[i]) return fail("a landmark");
  ++served;
  return 0;
}

static int selections() {
  for (uint32_t D : {6u, 15u})
    for (uint32_t K : {0u, 6u})
      for (uint32_t LM : {0u, 1u, 3u})
        for (bool perm : {false, true}) {
          const Case c = {D, K, LM, perm};
          const std::vector<uint32_t> none;
          for (bool caller : {false, true}) {
            const std::vector<uint32_t> lms = LM && !caller ? std::vector<uint32_t>{3, 0} : none;
            if (ask(c, {4, 0, 3}, lms, K != 0, caller, nullptr) || ask(c, {2}, none, false, caller, nullptr)) return 1;
            if (K && ask(c, none, none, true, caller, nullptr, true)) return 1;    // n = 0, NULL id pointers
            if (ask(c, none, none, false, caller, "nothing requested", true)) return 1;
            if (ask(c, {0, 3, 0}, none, false, caller, "pose 0 is repeated")) return 1;
            if (ask(c, {0, 1}, none, false, caller, "pose 1 is not an active pose")) return 1;
            if (ask(c, {5}, none, false, caller, "pose 5 is not an active pose")) return 1;
            if (ask(c, {0}, none, false, caller, "NULL argument", true)) return 1;
            if (!K && ask(c, {0}, none, true, caller, "include_calibration without calibration unknowns")) return 1;
            const uint32_t fit = (512 - K) / D;
            if (ask(c, std::vector<uint32_t>(fit, 0), none, K != 0, caller, "is repeated")) return 1;
            if (ask(c, std::vector<uint32_t>(fit + 1, 0), none, K != 0, caller, "columns requested, the limit is BA_HIP_")) return 1;
          }
          if (LM) {
            if (ask(c, {0}, {3, 0, 3}, false, false, "landmark 3 is repeated")) return 1;
            if (ask(c, {0}, {2}, false, false, "landmark 2 is not an active landmark")) return 1;
            if (ask(c, {0}, {4}, false, false, "landmark 4 is not an active landmark")) return 1;
          } else if (ask(c, {0}, {0}, false, false, "landmark 0 is not an active landmark")) {
            return 1;
          }
          if (LM == 1 && ask(c, std::vector<uint32_t>((512 - K) / D, 0), std::vector<uint32_t>(512 - K - (512 - K) / D * D + 1, 0),
                             K != 0, false, "513 columns requested, the limit is BA_HIP_JOINT_MAX_COLUMNS (512)"))
            return 1;
        }
  return 0;
}

static int guards() {
  using namespace bae;
  const int32_t upload[] = {kEvProblemChanged, kEvFinalizeBegins, kEvStructureRebuilt, kEvFinalizeSucceeded, kEvSolveBegins,
                            kEvMasksChanged, kEvLinearizeBegins, kEvLinearizeWritesA, kEvPatternBuilt, kEvSquareCleared,
                            kEvLinearizeSucceeded, kEvGnSolveBegins};
  const std::vector<int32_t> head(upload, upload + sizeof(upload) / sizeof(upload[0]));
  std::vector<int32_t> direct = head, pcg = head;
  for (int32_t ev : {kEvSolvedDirectly, kEvSelinvComputed, kEvStandaloneFactorisation, kEvSelinvReleased, kEvLinearizeBegins,
                     kEvLinearizeWritesA})
    direct.push_back(ev);
  for (int32_t ev : {kEvPcgRunBegins, kEvPcgRunFinishedCoarse, kEvSolvedByPcg, kEvStepAppliedTo1, kEvLinearizeBegins,
                     kEvLinearizeWritesA, kEvLinearizeSucceeded})
    pcg.push_back(ev);
  const char* names[] = {"kept_factor", "marginals", "pcg_panel", "check_solve", "get_S", "pcg_stats", "pcg_coarse_stats", "marginalize"};
  char msg[64];   // shorter than most messages: the copy must truncate
  for (const std::vector<int32_t>& round : {direct, pcg})
    for (size_t k = 0; k <= round.size(); ++k)
      for (const char* g : names)
        for (uint32_t facts = 0; facts < 32; ++facts)
          for (uint32_t flags = 0; flags < 16; ++flags)
            for (const char* noun : {(const char*)nullptr, "joint marginals"}) {
              const int rc = ba_hostcheck_guard((uint32_t)k, k ? round.data() : nullptr, g, "ba_hip_x", noun, facts, flags,
                                                flags & 8 ? 0.0 : 1e-8, flags & 1, msg, sizeof(msg));
              if (rc != 0 && rc != 1) return fail("a guard returned neither served nor refused");
              if ((rc == 1) != (msg[0] != 0) || strlen(msg) >= sizeof(msg)) return fail("a guard's message");
              ++(rc ? refused : served);
            }
  if (ba_hostcheck_guard(0, nullptr, "nothing", "w", nullptr, 0, 0, 0.5, 0, msg, sizeof(msg)) != -1000) return fail("unknown guard");
  return 0;
}

static int small_checks() {
  char msg[160];
  const double nan = std::nan("");
  const struct { int op; uint64_t u[3]; double d; int want; } rows[] = {
      {0, {0, 7, 7}, 0, 0}, {0, {0, 6, 7}, 0, 1}, {0, {1, 6, 7}, 0, 0}, {0, {0, 0, 0}, 0, 0},
      {1, {0, 1, 0}, 0.0, 1}, {1, {0, 1, 0}, 1.0, 1}, {1, {0, 1, 0}, nan, 1}, {1, {0, 1, 0}, 1e-9, 0}, {1, {2, 0, 0}, 1e-9, 1},
      {1, {2, 1, 0}, 1e-9, 0},
      {2, {0, 0, 0}, 0, 1}, {2, {1, 0, 0}, 0, 0}, {2, {16, 0, 0}, 0, 0}, {2, {17, 0, 0}, 0, 1},
      {3, {0, 512, 0}, 0, 1}, {3, {1, 512, 0}, 0, 0}, {3, {512, 512, 0}, 0, 0}, {3, {513, 512, 0}, 0, 1}};
  for (const auto& r : rows) {
    if (ba_hostcheck_request_check(r.op, "who", "the name", r.u, &r.d, msg, sizeof(msg)) != r.want) return fail("a small check");
    ++(r.want ? refused : served);
  }
  return 0;
}

int main() {
  if (selections() || guards() || small_checks()) return 1;
  printf("requests: %u served, %u refused: ok\n", served, refused);
  return 0;
}
