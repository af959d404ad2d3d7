// Stand-alone driver of the pose-pose lists and tile marks of structure.h (through ba_hostcheck_pose_pose_lists and
// ba_hostcheck_coupling_group_edges of hostcheck.cpp), for a sanitizer build:
//   make -C ba_amd/csrc ../lib/hostcheck_pose_pose_lists_asan && ba_amd/lib/hostcheck_pose_pose_lists_asan
// The graphs of tests/test_pose_pose_lists.py restated: PoseSize 6 and 15 with a pose that straddles tiles 0 / 1, reversed
// and duplicate pairs, p1 == p2, inactive ends, each residual kind absent in turn, no residual, no active pose, a
// non-identity ordering, prior cliques of 1 and 3, the calibration border over one and two tile rows, an unknown pose;
// and its graphs with empty tiles: six tiles of PoseSize 15 with one coupling of each kind alone in its off-band tile,
// borders near rows 128 and 192 that are the only source of their tiles, three pose groups.
// Every output buffer has exactly the size the entry fills.  Checked here: the return code and message, the counts, that
// the pattern EQUALS the one of an element-wise restatement (coupled active blocks, pose diagonals, the diagonal, the
// border rows; mirrored; reduced tile by tile), that it has the empty tiles the graph was built to have, and that every
// non-zero of S lies in a marked tile; the values of S are the subject of the pytest file.  Prints the totals and "ok".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

extern "C" int ba_hostcheck_pose_pose_lists(
    int D, int K, uint32_t P, const uint8_t* pose_active, uint32_t n_perm, const uint32_t* opt_of_natural, uint32_t nu,
    const uint32_t* un_pose, uint32_t nb, const uint32_t* bin_p1, const uint32_t* bin_p2, uint32_t ni, const uint32_t* imu_p1,
    const uint32_t* imu_p2, uint32_t nq, const uint32_t* prior_ptr, const uint32_t* prior_pose, const uint16_t* pose_mask,
    const double* pp_h, const double* pp_g, uint32_t ld, double* S_lower, double* rhs, uint8_t* tile_nz, uint32_t* counts,
    uint32_t* pp_ptr, uint32_t* pp_ent, char* msg, uint32_t cap);
extern "C" uint64_t ba_hostcheck_coupling_group_edges(int D, uint32_t P, const uint8_t* pose_active, uint32_t nb,
                                                      const uint32_t* bin_p1, const uint32_t* bin_p2, uint32_t ni,
                                                      const uint32_t* imu_p1, const uint32_t* imu_p2, uint32_t nq,
                                                      const uint32_t* prior_ptr, const uint32_t* prior_pose, uint64_t* edges,
                                                      uint64_t cap);

typedef std::vector<std::pair<uint32_t, uint32_t>> Pairs;
struct Graph {
  const char* name;
  int D, K;
  uint32_t P;
  std::vector<uint32_t> inactive, perm, unary;
  Pairs binary, imu;
  std::vector<std::vector<uint32_t>> priors;
  std::vector<std::pair<uint32_t, uint16_t>> masks;
  bool refused;   // an unknown pose: the builder's message is expected
  bool none_active = false;
  int empty_lower_tiles = -1;   // tiles (r, c <= r) the pattern must leave 0; -1: not stated
};

static unsigned long entries = 0, tiles = 0, empty_tiles = 0, edges_total = 0, refusals = 0;

static int fail(const char* graph, const char* what) {
  fprintf(stderr, "hostcheck_pose_pose_lists: %s: %s\n", graph, what);
  return 1;
}

static int run(const Graph& g) {
  std::vector<uint8_t> active(g.P, 1);
  if (g.none_active) active.assign(g.P, 0);
  for (uint32_t p : g.inactive) active[p] = 0;
  const uint32_t Pact = (uint32_t)std::count(active.begin(), active.end(), 1);
  std::vector<uint16_t> mask(g.P, 0);
  for (const auto& m : g.masks) mask[m.first] = m.second;
  std::vector<uint32_t> b1, b2, i1, i2, qptr(1, 0), qpose;
  for (const auto& p : g.binary) { b1.push_back(p.first); b2.push_back(p.second); }
  for (const auto& p : g.imu) { i1.push_back(p.first); i2.push_back(p.second); }
  for (const auto& q : g.priors) { qpose.insert(qpose.end(), q.begin(), q.end()); qptr.push_back((uint32_t)qpose.size()); }
  const uint32_t nres = (uint32_t)(g.unary.size() + b1.size() + i1.size());
  const uint32_t n = Pact * (uint32_t)g.D + (uint32_t)g.K, ld = std::max(64u, (n + 63) / 64 * 64), nt = ld / 64;
  std::vector<double> h((size_t)nres * 3 * 225), gr((size_t)nres * 30);
  for (size_t k = 0; k < h.size(); ++k) h[k] = 1.0 + (double)(k % 97);   // no zero: a placed element is a non-zero
  for (size_t k = 0; k < gr.size(); ++k) gr[k] = 1.0 + (double)(k % 31);
  std::vector<double> S((size_t)ld * ld), rhs(ld);
  std::vector<uint8_t> nz((size_t)nt * nt);
  std::vector<uint32_t> counts(5), pp_ptr((size_t)Pact + 1);
  char msg[64];
  // the number of entries is an output: first into a buffer for the most a graph can have, then into one of exactly that size
  std::vector<uint32_t> ent((size_t)2 * nres * 4);
  for (int pass = 0; pass < 2; ++pass) {
    const int rc = ba_hostcheck_pose_pose_lists(
        g.D, g.K, g.P, active.data(), (uint32_t)g.perm.size(), g.perm.data(), (uint32_t)g.unary.size(), g.unary.data(),
        (uint32_t)b1.size(), b1.data(), b2.data(), (uint32_t)i1.size(), i1.data(), i2.data(), (uint32_t)g.priors.size(),
        qptr.data(), qpose.data(), mask.data(), h.data(), gr.data(), ld, S.data(), rhs.data(), nz.data(), counts.data(),
        pp_ptr.data(), ent.data(), msg, sizeof(msg));
    if (g.refused) {
      if (rc != 1 || strcmp(msg, "pose-pose residual references an unknown pose") != 0) return fail(g.name, "the refusal");
      ++refusals;
      return 0;
    }
    if (rc != 0 || msg[0]) return fail(g.name, "refused");
    if (counts[0] != Pact || counts[1] != n || counts[2] != ld || counts[4] != nres || counts[3] > 2 * nres)
      return fail(g.name, "the counts");
    if (pp_ptr[Pact] != counts[3]) return fail(g.name, "pp_ptr does not end at the entry count");
    std::vector<uint32_t>((size_t)counts[3] * 4).swap(ent);
  }
  entries += counts[3];
  // the pattern, element by element
  {
    std::vector<int64_t> opt(g.P, -1);
    uint32_t k = 0;
    for (uint32_t p = 0; p < g.P; ++p)
      if (active[p]) { opt[p] = g.perm.empty() ? k : g.perm[k]; ++k; }
    std::vector<uint8_t> el((size_t)ld * ld, 0);
    const uint32_t D = (uint32_t)g.D, np = Pact * D;
    auto block = [&](int64_t a, int64_t b) {
      if (a < 0 || b < 0) return;
      for (uint32_t r = 0; r < D; ++r)
        for (uint32_t c = 0; c < D; ++c) el[((size_t)a * D + r) * ld + (size_t)b * D + c] = 1;
    };
    for (const auto& p : g.binary) block(opt[p.first], opt[p.second]);
    for (const auto& p : g.imu) block(opt[p.first], opt[p.second]);
    for (const auto& q : g.priors)
      for (uint32_t a : q)
        for (uint32_t b : q) block(opt[a], opt[b]);
    for (uint32_t p = 0; p < Pact; ++p) block(p, p);
    for (uint32_t r = 0; r < ld; ++r) el[(size_t)r * ld + r] = 1;
    for (uint32_t r = np; r < n; ++r)
      for (uint32_t c = 0; c < n; ++c) el[(size_t)r * ld + c] = 1;
    std::vector<uint8_t> want((size_t)nt * nt, 0);
    for (uint32_t r = 0; r < ld; ++r)
      for (uint32_t c = 0; c < ld; ++c)
        if (el[(size_t)r * ld + c]) want[(size_t)(r / 64) * nt + c / 64] = want[(size_t)(c / 64) * nt + r / 64] = 1;
    if (want != nz) return fail(g.name, "the pattern is not the element-wise one");
  }
  int empty = 0;
  for (uint32_t r = 0; r < nt; ++r)
    for (uint32_t c = 0; c < nt; ++c) {
      if (nz[(size_t)r * nt + c] != nz[(size_t)c * nt + r]) return fail(g.name, "the pattern is not symmetric");
      tiles += nz[(size_t)r * nt + c];
      empty += c <= r && !nz[(size_t)r * nt + c];
    }
  if (g.empty_lower_tiles >= 0 && empty != g.empty_lower_tiles) return fail(g.name, "the number of empty tiles");
  empty_tiles += (unsigned long)empty;
  for (uint32_t r = 0; r < ld; ++r)
    for (uint32_t c = 0; c < ld; ++c)
      if (S[(size_t)r * ld + c] != 0.0 && !nz[(size_t)(r / 64) * nt + c / 64]) return fail(g.name, "a non-zero outside the pattern");
  std::vector<uint64_t> ed(b1.size() + i1.size() + qpose.size() * qpose.size());
  const uint64_t ne = ba_hostcheck_coupling_group_edges(g.D, g.P, active.data(), (uint32_t)b1.size(), b1.data(), b2.data(),
                                                        (uint32_t)i1.size(), i1.data(), i2.data(), (uint32_t)g.priors.size(),
                                                        qptr.data(), qpose.data(), ed.data(), ed.size());
  if (ne > ed.size()) return fail(g.name, "more group edges than couplings");
  edges_total += (unsigned long)ne;
  return 0;
}

int main() {
  const Pairs bin6 = {{1, 2}, {5, 4}, {1, 2}, {2, 1}, {6, 6}, {3, 4}, {4, 7}, {3, 7}, {12, 0}, {13, 12}, {12, 14}, {15, 8}};
  const Pairs imu6 = {{8, 9}, {9, 10}, {10, 11}, {11, 12}, {12, 13}, {7, 8}, {13, 13}};
  const std::vector<uint32_t> un6 = {0, 12, 3, 12, 15};
  const std::vector<std::vector<uint32_t>> pri6 = {{5}, {0, 12, 15}, {4, 3, 9}};
  const std::vector<std::pair<uint32_t, uint16_t>> m6 = {{12, 0x7}, {0, 0x38}, {2, 0x5}, {3, 0x3f}};
  const Graph d6 = {"d6", 6, 0, 16, {3, 7}, {}, un6, bin6, imu6, pri6, m6, false};
  std::vector<Graph> graphs = {d6};
  auto variant = [&](const char* name, auto&& change) {
    Graph g = d6;
    g.name = name;
    change(g);
    graphs.push_back(g);
  };
  variant("d6 reversed", [](Graph& g) { for (uint32_t k = 0; k < 14; ++k) g.perm.push_back(13 - k); });
  variant("d6 shuffled", [](Graph& g) { g.perm = {5, 0, 13, 2, 9, 7, 11, 1, 12, 3, 6, 10, 4, 8}; });
  variant("no unary", [](Graph& g) { g.unary.clear(); });
  variant("no binary", [](Graph& g) { g.binary.clear(); });
  variant("no imu", [](Graph& g) { g.imu.clear(); });
  variant("no residuals", [](Graph& g) { g.unary.clear(); g.binary.clear(); g.imu.clear(); g.priors.clear(); });
  variant("no active pose", [](Graph& g) { g.none_active = true; g.priors.clear(); });
  variant("unknown unary pose", [](Graph& g) { g.unary.push_back(16); g.refused = true; });
  variant("unknown binary pose", [](Graph& g) { g.binary.push_back({1, 21}); g.refused = true; });
  variant("unknown imu pose", [](Graph& g) { g.imu.insert(g.imu.begin(), {16, 1}); g.refused = true; });
  graphs.push_back({"d15", 15, 0, 8, {1}, {3, 6, 0, 5, 1, 4, 2}, {5, 1, 0}, {{5, 0}, {2, 5}, {5, 6}, {6, 5}, {1, 5}, {4, 4}},
                    {{0, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 6}, {6, 7}, {7, 6}, {3, 1}, {3, 4}}, {{7}, {5, 0, 1}},
                    {{5, 0x4003}, {0, 0x0700}, {6, 0x1}}, false});
  // three tiles; (2, 0) from the binary residual (23, 0) alone, the rest in the band of the straddling poses 10 and 21
  graphs.push_back({"far tile", 6, 0, 24, {}, {}, {23}, {{23, 0}, {11, 10}}, {{21, 20}}, {{2}, {20, 12, 13}}, {}, false, false, 0});
  // six tiles of PoseSize 15 (pose 24 inactive): (2, 0) binary; (4, 2), (5, 2) binary with a straddling row pose; (3, 1)
  // inertial; (5, 0), (5, 1) inertial with a straddling column pose; (4, 0) prior; (3, 0), (4, 1), (5, 3) empty
  const Graph t15 = {"tiles d15", 15, 0, 25, {24}, {}, {3, 24}, {{9, 0}, {21, 10}, {24, 2}}, {{14, 5}, {23, 4}},
                     {{18, 1}, {6}, {24, 13, 14}}, {{21, 0x11}, {10, 0x4000}}, false, false, 3};
  graphs.push_back(t15);
  for (int kind = 0; kind < 3; ++kind) {   // each kind gone: its tiles go with it
    Graph g = t15;
    g.name = kind == 0 ? "tiles d15, no binary" : kind == 1 ? "tiles d15, no imu" : "tiles d15, no priors";
    if (kind == 0) g.binary.clear();
    if (kind == 1) g.imu.clear();
    if (kind == 2) g.priors.clear();
    g.empty_lower_tiles = 3 + (kind == 2 ? 1 : 3);
    graphs.push_back(g);
  }
  {
    Graph g = t15;
    g.name = "tiles d15 shuffled";
    g.perm = {17, 3, 22, 8, 0, 13, 19, 5, 11, 23, 1, 15, 7, 20, 2, 10, 16, 4, 21, 9, 14, 6, 18, 12};
    g.empty_lower_tiles = -1;
    graphs.push_back(g);
  }
  graphs.push_back({"border, two tile rows", 6, 6, 12, {4, 9}, {}, {0}, {{11, 0}, {3, 4}}, {{1, 2}}, {}, {}, false});
  graphs.push_back({"border, one tile row", 6, 6, 12, {4}, {}, {0}, {{11, 0}, {3, 4}}, {{1, 2}}, {}, {}, false});
  graphs.push_back({"border only", 6, 6, 11, {}, {}, {}, {}, {}, {}, {}, false});
  // borders that are the only source of their tiles: np = 126 (tile rows 1 and 2) and 132 (row 2) at PoseSize 6, np = 189
  // (rows 2 and 3) and 198 (row 3; tile (2, 0) stays empty) at PoseSize 9
  graphs.push_back({"border d6, rows 1 and 2", 6, 6, 21, {}, {}, {0}, {{1, 0}}, {}, {}, {}, false, false, 0});
  graphs.push_back({"border d6, row 2", 6, 6, 22, {}, {}, {}, {}, {{1, 0}}, {}, {}, false, false, 0});
  graphs.push_back({"border d9, rows 2 and 3", 9, 6, 21, {}, {}, {20}, {}, {}, {}, {}, false, false, 0});
  graphs.push_back({"border d9, row 3", 9, 6, 22, {}, {}, {}, {{2, 1}}, {}, {}, {}, false, false, 1});
  // 70 poses in groups of 32 (one inactive), seven tiles: the only graph here with more than one group, 9 group edges
  graphs.push_back({"three groups", 6, 0, 70, {40}, {}, {69}, {{0, 69}, {69, 0}, {0, 40}, {1, 2}, {33, 31}}, {{31, 32}, {64, 65}},
                    {{0, 35, 69}, {40, 1, 68}}, {}, false});
  for (const Graph& g : graphs)
    if (run(g)) return 1;
  if (edges_total != 9) return fail("three groups", "the group edges");
  printf("pose-pose lists: %zu graphs, %lu scatter entries, %lu marked tiles, %lu empty lower tiles, %lu group edges, %lu refusals: ok\n",
         graphs.size(), entries, tiles, empty_tiles, edges_total, refusals);
  return 0;
}
