// Fill-reducing ordering of the poses of the reduced camera system (ba_hip_set_pose_ordering), and the
// symbolic tile elimination shared with the factorisation (factor_tile_pattern) and the
// factor_tile_products statistic.  Plain C++17, no HIP: the CPU harness (hostcheck.cpp,
// tests/test_pose_ordering.py) compiles the same code.
//
// Tile alignment.  The factorisation works on 64x64 tiles, and a tile of D-row poses holds 64 / D of
// them.  Permuting single poses scatters unrelated poses into one tile and makes the tile work worse,
// not better.  The ordering therefore permutes GROUPS of G = lcm(D, 64) / D consecutive poses (32 for
// D = 6, 64 for D = 9 and 15): the rows of a group start on a tile boundary and span tpg = G D / 64
// whole tiles.  A group keeps its internal order; the partial last group (Pact mod G poses) and the
// calibration border (rows np .. n - 1) stay behind all full groups.
//
// Selection.  Heuristics can lose against natural order on some graphs, so every candidate ordering
// is scored by the exact tile products of the symbolic LDL^T on the tile pattern it implies, and the
// smallest wins (ties go to the earlier candidate; natural is candidate 0).  The pattern is derived from
// the group graph: every coupled pair of groups counts as a full tpg x tpg tile block, an upper bound
// of the exact pattern that is the same model for every candidate.
//
// Candidates: 0 natural; 1 minimum degree on the group graph + elimination-tree postorder; 2 the same on
// pairs of consecutive groups; 3 nested dissection by recursive BFS level-set bisection.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

namespace bae {

// ---- symbolic elimination at tile granularity ---------------------------------------------------------
// nz: nt x nt bytes, symmetric pattern of S on input; on output the LOWER pattern of the factor L
// (row-major, nz[i * nt + k] = L(i, k) != 0 for k <= i, 0 above the diagonal).  Right-looking:
// L(i, j) becomes nonzero when L(i, k) and L(j, k) are, k < j <= i.
inline void tile_symbolic_factor(std::vector<uint8_t>& nz, uint32_t nt) {
  const size_t W = (nt + 63) / 64;
  // column k as a bit set of its rows i >= k
  std::vector<uint64_t> col((size_t)nt * W, 0);
  for (uint32_t i = 0; i < nt; ++i)
    for (uint32_t k = 0; k <= i; ++k)
      if (nz[(size_t)i * nt + k] || nz[(size_t)k * nt + i]) col[(size_t)k * W + i / 64] |= 1ull << (i % 64);
  for (uint32_t k = 0; k < nt; ++k) {
    const uint64_t* ck = &col[(size_t)k * W];
    for (size_t w = (k + 1) / 64; w < W; ++w) {
      uint64_t bits = ck[w];
      if (w == (k + 1) / 64) bits &= ~0ull << ((k + 1) % 64);
      while (bits) {
        const uint32_t j = (uint32_t)(w * 64 + __builtin_ctzll(bits));
        bits &= bits - 1;
        // column j gains every row of column k at or below j
        uint64_t* cj = &col[(size_t)j * W];
        cj[j / 64] |= ck[j / 64] & (~0ull << (j % 64));
        for (size_t u = j / 64 + 1; u < W; ++u) cj[u] |= ck[u];
      }
    }
  }
  for (uint32_t i = 0; i < nt; ++i)
    for (uint32_t k = 0; k < nt; ++k)
      nz[(size_t)i * nt + k] = (k <= i) ? (uint8_t)((col[(size_t)k * W + i / 64] >> (i % 64)) & 1) : 0;
}

// 64x64x64 tile products of the tile-sparse LDL^T on the factor's lower pattern: column k with m_k
// structurally nonzero tiles below the diagonal costs m_k (m_k + 1) / 2 update products, m_k / 2
// substitution products (a triangular 64x64 solve is half a product) and m_k + 1 for the rhs row.
inline uint64_t factor_tile_products(const std::vector<uint8_t>& nzL, uint32_t nt) {
  uint64_t total = 0;
  for (uint64_t k = 0; k < nt; ++k) {
    uint64_t m = 0;
    for (uint64_t i = k + 1; i < nt; ++i) m += nzL[i * nt + k] ? 1 : 0;
    total += m * (m + 1) / 2 + (m + 1) / 2 + m + 1;
  }
  return total;
}

// ---- pose ordering ----------------------------------------------------------------------------------------
enum { kOrderNatural = 0, kOrderAuto = 1, kOrderUser = 2 };
static const int kOrderCandidates = 4;

inline uint32_t gcd_u32(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }
// poses per tile-aligned group: lcm(D, 64) / D
inline uint32_t pose_group_size(int D) { return D > 0 ? 64u / gcd_u32((uint32_t)D, 64u) : 1u; }

struct OrderingResult {
  int candidate = 0;                        // index of the candidate kept
  uint32_t G = 1;                           // poses per group
  uint64_t products[kOrderCandidates] = {}; // model tile products per candidate (0: not evaluated)
};

namespace detail {

// group graph as adjacency bit sets (ng x ng), symmetric, no self loops
struct BitGraph {
  uint32_t n = 0;
  size_t W = 0;
  std::vector<uint64_t> b;
  void init(uint32_t n_) { n = n_; W = (n + 63) / 64; b.assign((size_t)n * W, 0); }
  uint64_t* row(uint32_t i) { return &b[(size_t)i * W]; }
  const uint64_t* row(uint32_t i) const { return &b[(size_t)i * W]; }
  bool has(uint32_t i, uint32_t j) const { return (row(i)[j / 64] >> (j % 64)) & 1; }
  void set(uint32_t i, uint32_t j) { row(i)[j / 64] |= 1ull << (j % 64); }
};

inline BitGraph bit_graph(uint32_t ng, const std::vector<uint32_t>& ptr, const std::vector<uint32_t>& adj) {
  BitGraph g;
  g.init(ng);
  for (uint32_t i = 0; i < ng; ++i)
    for (uint32_t e = ptr[i]; e < ptr[i + 1]; ++e)
      if (adj[e] != i && adj[e] < ng) { g.set(i, adj[e]); g.set(adj[e], i); }
  return g;
}

// Minimum degree on the explicit elimination graph; the `fixed` nodes (>= n_free) are never chosen and
// come last in their own order.  Ties: the smallest index.  Returns order[position] = node.
inline std::vector<uint32_t> min_degree(BitGraph g, uint32_t n_free) {
  const uint32_t n = g.n;
  std::vector<uint32_t> order;
  std::vector<uint8_t> gone(n, 0);
  std::vector<uint32_t> deg(n, 0), nb;
  for (uint32_t i = 0; i < n; ++i)
    for (size_t w = 0; w < g.W; ++w) deg[i] += (uint32_t)__builtin_popcountll(g.row(i)[w]);
  for (uint32_t step = 0; step < n_free; ++step) {
    uint32_t best = n;
    for (uint32_t i = 0; i < n_free; ++i)
      if (!gone[i] && (best == n || deg[i] < deg[best])) best = i;
    order.push_back(best);
    gone[best] = 1;
    nb.clear();
    const uint64_t* rb = g.row(best);
    for (size_t w = 0; w < g.W; ++w)
      for (uint64_t bits = rb[w]; bits; bits &= bits - 1) nb.push_back((uint32_t)(w * 64 + __builtin_ctzll(bits)));
    // the neighbours become a clique; `best` leaves the graph
    for (uint32_t a : nb) {
      uint64_t* ra = g.row(a);
      for (size_t w = 0; w < g.W; ++w) ra[w] |= rb[w];
      ra[a / 64] &= ~(1ull << (a % 64));
      ra[best / 64] &= ~(1ull << (best % 64));
      deg[a] = 0;
      for (size_t w = 0; w < g.W; ++w) deg[a] += (uint32_t)__builtin_popcountll(ra[w]);
    }
  }
  for (uint32_t i = n_free; i < n; ++i) order.push_back(i);
  return order;
}

// Elimination-tree postorder of an ordering (same fill, subtrees contiguous); fixed tail unchanged.
inline std::vector<uint32_t> etree_postorder(const BitGraph& g, const std::vector<uint32_t>& order, uint32_t n_free) {
  const uint32_t n = g.n;
  std::vector<uint32_t> pos(n);
  for (uint32_t p = 0; p < n; ++p) pos[order[p]] = p;
  // symbolic elimination in the permuted numbering: parent(j) = first off-diagonal row of column j
  BitGraph h;
  h.init(n);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < n; ++j)
      if (g.has(i, j)) h.set(pos[i], pos[j]);
  std::vector<uint32_t> parent(n, n);
  for (uint32_t k = 0; k < n; ++k) {
    uint64_t* rk = h.row(k);
    uint32_t first = n;
    for (size_t w = (k + 1) / 64; w < h.W && first == n; ++w) {
      uint64_t bits = rk[w];
      if (w == (k + 1) / 64) bits &= ~0ull << ((k + 1) % 64);
      if (bits) first = (uint32_t)(w * 64 + __builtin_ctzll(bits));
    }
    if (first == n) continue;
    parent[k] = first;
    uint64_t* rp = h.row(first);
    for (size_t w = 0; w < h.W; ++w) rp[w] |= rk[w];
    for (uint32_t x = 0; x <= first; ++x) rp[x / 64] &= ~(1ull << (x % 64));  // keep rows below `first` only
  }
  std::vector<std::vector<uint32_t>> kids(n + 1);
  for (uint32_t k = 0; k < n_free; ++k) kids[parent[k] < n_free ? parent[k] : n].push_back(k);
  std::vector<uint32_t> post;
  std::vector<std::pair<uint32_t, size_t>> stack;
  stack.push_back({n, 0});
  while (!stack.empty()) {
    auto& top = stack.back();
    if (top.second < kids[top.first].size()) {
      const uint32_t c = kids[top.first][top.second++];
      stack.push_back({c, 0});
    } else {
      if (top.first != n) post.push_back(order[top.first]);
      stack.pop_back();
    }
  }
  for (uint32_t p = n_free; p < n; ++p) post.push_back(order[p]);
  return post;
}

// Nested dissection: BFS level sets from a pseudo-peripheral node, the middle level is the separator,
// parts first, separator last; parts of at most `leaf` nodes keep their natural order.
inline void dissect(const BitGraph& g, std::vector<uint32_t> nodes, std::vector<uint32_t>& out, uint32_t leaf) {
  if (nodes.size() <= leaf) { std::sort(nodes.begin(), nodes.end()); out.insert(out.end(), nodes.begin(), nodes.end()); return; }
  std::vector<int32_t> lvl(g.n, -2);
  for (uint32_t v : nodes) lvl[v] = -1;
  auto bfs = [&](uint32_t s, std::vector<uint32_t>& seq) {
    for (uint32_t v : nodes) lvl[v] = -1;
    seq.clear();
    seq.push_back(s);
    lvl[s] = 0;
    for (size_t q = 0; q < seq.size(); ++q) {
      const uint32_t v = seq[q];
      const uint64_t* r = g.row(v);
      for (size_t w = 0; w < g.W; ++w)
        for (uint64_t bits = r[w]; bits; bits &= bits - 1) {
          const uint32_t u = (uint32_t)(w * 64 + __builtin_ctzll(bits));
          if (lvl[u] == -1) { lvl[u] = lvl[v] + 1; seq.push_back(u); }
        }
    }
  };
  std::vector<uint32_t> seq;
  uint32_t s = *std::min_element(nodes.begin(), nodes.end());
  bfs(s, seq);
  if (seq.size() < nodes.size()) {  // disconnected: each component on its own
    std::vector<uint32_t> comp(seq), rest;
    for (uint32_t v : nodes) if (lvl[v] == -1) rest.push_back(v);
    dissect(g, comp, out, leaf);
    dissect(g, rest, out, leaf);
    return;
  }
  for (int it = 0; it < 4; ++it) {  // pseudo-peripheral: restart from the last node of the deepest level
    const uint32_t far = seq.back();
    const int32_t depth = lvl[far];
    std::vector<uint32_t> s2;
    bfs(far, s2);
    if (lvl[s2.back()] <= depth) { bfs(far, seq); break; }
    seq.swap(s2);
  }
  const int32_t depth = lvl[seq.back()];
  if (depth < 2) { std::sort(nodes.begin(), nodes.end()); out.insert(out.end(), nodes.begin(), nodes.end()); return; }
  // the level that splits the nodes closest to half
  std::vector<uint32_t> cnt(depth + 1, 0);
  for (uint32_t v : nodes) cnt[lvl[v]]++;
  int32_t mid = 1;
  {
    uint32_t below = 0, best = ~0u;
    for (int32_t d = 1; d < depth; ++d) {
      below += cnt[d - 1];
      const uint32_t above = (uint32_t)nodes.size() - below - cnt[d];
      const uint32_t diff = below > above ? below - above : above - below;
      if (diff < best) { best = diff; mid = d; }
    }
  }
  std::vector<uint32_t> a, b, sep;
  for (uint32_t v : nodes) (lvl[v] < mid ? a : lvl[v] > mid ? b : sep).push_back(v);
  dissect(g, a, out, leaf);
  dissect(g, b, out, leaf);
  std::sort(sep.begin(), sep.end());
  out.insert(out.end(), sep.begin(), sep.end());
}

}  // namespace detail

// Model tile products of a group order (order[position] = group): the group graph expanded to tiles
// (tpg per full group, a coupled pair = a full block), the tail (partial group + calibration border)
// behind, the border rows dense.
inline uint64_t group_order_products(uint32_t Pact, int D, uint32_t K, const std::vector<uint32_t>& gptr,
                                     const std::vector<uint32_t>& gadj, const std::vector<uint32_t>& order) {
  const uint32_t G = pose_group_size(D), nfull = Pact / G, ng = (Pact + G - 1) / G;
  const uint32_t tpg = G * (uint32_t)D / 64;
  const uint32_t np = Pact * (uint32_t)D, n = np + K;
  const uint32_t nt = std::max<uint32_t>((n + 63) / 64, 1);
  std::vector<uint32_t> pos(ng);
  for (uint32_t p = 0; p < ng; ++p) pos[order[p]] = p;
  auto tiles = [&](uint32_t grp, uint32_t& t0, uint32_t& t1) {  // [t0, t1) tiles of group grp at its position
    if (grp < nfull) { t0 = pos[grp] * tpg; t1 = t0 + tpg; }
    else { t0 = nfull * tpg; t1 = (np + 63) / 64; }
  };
  std::vector<uint8_t> nz((size_t)nt * nt, 0);
  auto block = [&](uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1) {
    for (uint32_t r = r0; r < r1; ++r)
      for (uint32_t c = c0; c < c1; ++c) { nz[(size_t)r * nt + c] = 1; nz[(size_t)c * nt + r] = 1; }
  };
  for (uint32_t grp = 0; grp < ng; ++grp) {
    uint32_t a0, a1;
    tiles(grp, a0, a1);
    block(a0, a1, a0, a1);
    for (uint32_t e = gptr[grp]; e < gptr[grp + 1]; ++e) {
      if (gadj[e] >= ng) continue;
      uint32_t b0, b1;
      tiles(gadj[e], b0, b1);
      block(a0, a1, b0, b1);
    }
  }
  if (K) block(np / 64, nt, 0, nt);
  for (uint32_t t = 0; t < nt; ++t) nz[(size_t)t * nt + t] = 1;
  tile_symbolic_factor(nz, nt);
  return factor_tile_products(nz, nt);
}

// Chooses opt_of_natural[Pact] (natural optimisation index -> factorised index) from the group graph:
// CSR over ng = ceil(Pact / G) groups (g = natural opt index / G), symmetric, self loops ignored.
inline void choose_pose_ordering(uint32_t Pact, int D, uint32_t K, const std::vector<uint32_t>& gptr,
                                 const std::vector<uint32_t>& gadj, std::vector<uint32_t>& opt_of_natural,
                                 OrderingResult* res) {
  OrderingResult r;
  const uint32_t G = pose_group_size(D), nfull = Pact / G, ng = (Pact + G - 1) / G;
  r.G = G;
  std::vector<uint32_t> best(ng);
  std::iota(best.begin(), best.end(), 0u);
  if (nfull >= 2) {
    const detail::BitGraph g = detail::bit_graph(ng, gptr, gadj);
    std::vector<std::vector<uint32_t>> cand(kOrderCandidates);
    cand[0] = best;
    cand[1] = detail::etree_postorder(g, detail::min_degree(g, nfull), nfull);
    {
      // pairs of consecutive full groups (2 G poses); an odd last full group is a node of its own
      const uint32_t nc = (nfull + 1) / 2, ncg = nc + (ng - nfull);
      std::vector<uint32_t> cp(ncg + 1, 0), ca;
      auto coarse = [&](uint32_t x) { return x < nfull ? x / 2 : nc + (x - nfull); };
      std::vector<std::vector<uint32_t>> nb(ncg);
      for (uint32_t x = 0; x < ng; ++x)
        for (uint32_t e = gptr[x]; e < gptr[x + 1]; ++e)
          if (gadj[e] < ng && coarse(gadj[e]) != coarse(x)) nb[coarse(x)].push_back(coarse(gadj[e]));
      for (uint32_t c = 0; c < ncg; ++c) {
        std::sort(nb[c].begin(), nb[c].end());
        nb[c].erase(std::unique(nb[c].begin(), nb[c].end()), nb[c].end());
        cp[c + 1] = cp[c] + (uint32_t)nb[c].size();
        ca.insert(ca.end(), nb[c].begin(), nb[c].end());
      }
      const detail::BitGraph gc = detail::bit_graph(ncg, cp, ca);
      const std::vector<uint32_t> oc = detail::etree_postorder(gc, detail::min_degree(gc, nc), nc);
      for (uint32_t c : oc) {
        if (c >= nc) continue;
        cand[2].push_back(2 * c);
        if (2 * c + 1 < nfull) cand[2].push_back(2 * c + 1);
      }
      for (uint32_t x = nfull; x < ng; ++x) cand[2].push_back(x);
    }
    {
      std::vector<uint32_t> nodes(nfull);
      std::iota(nodes.begin(), nodes.end(), 0u);
      detail::dissect(g, nodes, cand[3], 4);
      for (uint32_t x = nfull; x < ng; ++x) cand[3].push_back(x);
    }
    for (int c = 0; c < kOrderCandidates; ++c) {
      r.products[c] = group_order_products(Pact, D, K, gptr, gadj, cand[c]);
      if (r.products[c] < r.products[r.candidate]) r.candidate = c;
    }
    best = cand[r.candidate];
  } else {
    r.products[0] = group_order_products(Pact, D, K, gptr, gadj, best);
  }
  // group order -> pose permutation
  opt_of_natural.assign(Pact, 0);
  for (uint32_t p = 0; p < ng; ++p) {
    const uint32_t grp = best[p];
    for (uint32_t q = 0; q < G && grp * G + q < Pact; ++q) opt_of_natural[grp * G + q] = p * G + q;
  }
  if (res) *res = r;
}

// Symmetric CSR of a group graph from an edge list of (group a, group b) pairs; duplicates and self loops
// dropped, neighbours ascending.
inline void group_graph_csr(uint32_t ng, std::vector<uint64_t> edges, std::vector<uint32_t>& ptr,
                            std::vector<uint32_t>& adj) {
  std::vector<uint64_t> both;
  both.reserve(2 * edges.size());
  for (uint64_t e : edges) {
    const uint32_t a = (uint32_t)(e >> 32), b = (uint32_t)e;
    if (a == b || a >= ng || b >= ng) continue;
    both.push_back((uint64_t)a << 32 | b);
    both.push_back((uint64_t)b << 32 | a);
  }
  std::sort(both.begin(), both.end());
  both.erase(std::unique(both.begin(), both.end()), both.end());
  ptr.assign((size_t)ng + 1, 0);
  adj.resize(both.size());
  for (size_t i = 0; i < both.size(); ++i) { ptr[(both[i] >> 32) + 1]++; adj[i] = (uint32_t)both[i]; }
  for (uint32_t g = 0; g < ng; ++g) ptr[g + 1] += ptr[g];
}

}  // namespace bae
