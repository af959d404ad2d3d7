// Ownership map, message plan and every derived table of the distributed reduced solve
// — plain host C++, no device code: dist_solve.hip uploads the tables and executes the plan, ba_hip_dist_plan_stats
// only counts its bytes, hostcheck.cpp evaluates the same functions on the CPU (tests/test_dist_plan.py,
// tests/test_dist_tables.py).  Replaces nothing in the reference (arpg/ba is single-process); what is distributed is
// CalculateGn, /root/reference/src/BundleAdjuster.cpp:748-833.
//
// The lower triangle of S is cut into BLOCKS of G x G 64-tiles (G = the outer panel width KOUT of the
// single-GPU factorisation, so a column of blocks is one outer panel).  Block row / column b has the
// class b mod T, and the owner of block (bi, bc), bi >= bc, is tbl[class(bi)][class(bc)]:
//
//   tri   T(T-1)/2 "cross" ranks own the blocks of one unordered class pair {a, b}, T/2 "diagonal" ranks
//         the blocks (a, a) of two classes — N = T^2/2 ranks (2, 8, 18): every rank multiplies rows of only
//         TWO classes, so it receives 2/T of the factor (half of it at N = 8), and the blocks of a pair are
//         balanced to one unit of work per rank;
//   grid  Pr x Pc block-cyclic, tbl[a][b] = (a mod Pr) Pc + (b mod Pc), T = lcm(Pr, Pc);
//   col   tbl[a][b] = b (T = N): round-robin column panels — every rank receives the whole factor;
//   row   tbl[a][b] = a (T = N): round-robin block rows — the whole factor again, but a block row never
//         changes hands, so no bulk message sits between two consecutive panels of a row.
//
// Per panel J (tile columns [c0, c1)):
//   1. the owner of block (J, J) factorises the SQUARE (its G diagonal tiles, the tiles between them and
//      the rhs row) and broadcasts it with its factor packets — the only message every rank waits for;
//   2. every rank runs the panel's substitution / in-panel updates on the row tiles it owns below the
//      square; block J+1 first — its rows are the URGENT message (the next square needs them);
//   3. the rows of a block of class a go to the ranks that multiply class a (needs[q][a]), point to
//      point over xGMI: urgent ones on the chain communicator, the rest on the side communicator;
//   4. trailing updates of the tiles a rank owns.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace bae {

static const uint32_t kOwnMaxT = 16;

// Passed by value to the update kernels (plain data).
struct OwnMap {
  uint32_t n, rank, G, T, skip_rhs;
  uint8_t tbl[kOwnMaxT][kOwnMaxT];
  // k_update128<false, true> only (distributed bulk updates): the (block row, block column) pairs this rank owns
  // right of the next panel, G/2 x G/2 128-blocks each — the launch holds just these instead of the whole trailing
  // triangle with 1 - 1/N of its workgroups leaving at the ownership test.  Two 32-bit halves of the device address
  // (plain data for the host-only builds of this header).
  uint32_t pairs_lo, pairs_hi;
};

// Does this launch touch tile (i, c)?  i == nblk is the rhs row; its segment over block column bc rides
// with the diagonal block (bc, bc).  n <= 1: everything (single GPU).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool own_tile(const OwnMap& m, uint32_t i, uint32_t c, uint32_t nblk) {
  if (i == nblk && m.skip_rhs) return false;
  if (m.n <= 1) return true;
  const uint32_t cc = (c / m.G) % m.T;
  const uint32_t rc = (i == nblk) ? cc : (i / m.G) % m.T;
  return m.tbl[rc][cc] == m.rank;
}

inline OwnMap own_map_single() {
  OwnMap m = {};
  m.n = 1; m.rank = 0; m.G = 1; m.T = 1; m.skip_rhs = 0;
  return m;
}

// layout: "auto" | "tri" | "grid" | "col" | "row".  False (with *why) if it does not exist for nranks.
inline bool build_own_map(uint32_t nranks, const char* layout, uint32_t G, OwnMap* out, std::string* name,
                          std::string* why = nullptr) {
  OwnMap m = {};
  m.n = nranks; m.rank = 0; m.G = G ? G : 1; m.skip_rhs = 0;
  std::string lay = layout && *layout ? layout : "auto";
  auto tri_T = [&](uint32_t n) -> uint32_t {
    for (uint32_t t = 2; t <= kOwnMaxT; t += 2)
      if (t * t / 2 == n) return t;
    return 0;
  };
  if (nranks <= 1) {
    *out = own_map_single();
    out->G = m.G;
    if (name) *name = "single";
    return true;
  }
  if (lay == "auto") lay = tri_T(nranks) ? "tri" : "grid";
  if (lay == "tri") {
    const uint32_t T = tri_T(nranks);
    if (!T) { if (why) *why = "layout tri needs T*T/2 ranks (2, 8, 18, ...)"; return false; }
    m.T = T;
    uint32_t r = 0;
    for (uint32_t a = 0; a < T; ++a)
      for (uint32_t b = a + 1; b < T; ++b) { m.tbl[a][b] = m.tbl[b][a] = (uint8_t)r; ++r; }
    for (uint32_t k = 0; k < T / 2; ++k) { m.tbl[2 * k][2 * k] = m.tbl[2 * k + 1][2 * k + 1] = (uint8_t)(r + k); }
  } else if (lay == "grid") {
    uint32_t pr = 1;
    for (uint32_t d = 1; d * d <= nranks; ++d)
      if (nranks % d == 0) pr = d;
    const uint32_t pc = nranks / pr;
    uint32_t T = pc;
    while (T % pr) T += pc;
    if (T > kOwnMaxT) { if (why) *why = "layout grid: lcm(Pr, Pc) exceeds the class limit"; return false; }
    m.T = T;
    for (uint32_t a = 0; a < T; ++a)
      for (uint32_t b = 0; b < T; ++b) m.tbl[a][b] = (uint8_t)((a % pr) * pc + (b % pc));
  } else if (lay == "col" || lay == "row") {
    if (nranks > kOwnMaxT) { if (why) *why = "more ranks than classes"; return false; }
    m.T = nranks;
    for (uint32_t a = 0; a < m.T; ++a)
      for (uint32_t b = 0; b < m.T; ++b) m.tbl[a][b] = (uint8_t)(lay == "col" ? b : a);
  } else {
    if (why) *why = "unknown layout " + lay;
    return false;
  }
  *out = m;
  if (name) *name = lay;
  return true;
}

struct DistMsg {
  uint32_t panel, src;
  uint32_t first, count;        // tile list: tiles[first, first + count)
  std::vector<uint32_t> dst;    // receivers (never src, except the single-rank self test)
  bool urgent;
};

struct DistPanel {
  uint32_t c0, c1, diag_owner;
  // per rank: the row tiles it owns below the square — block J+1 (urgent) / the others — as ranges of `tiles`
  std::vector<uint32_t> own_u_first, own_u_count, own_r_first, own_r_count;
  std::vector<uint32_t> msgs;   // indices into DistPlan::msgs; urgent ones first
  // per rank: does its update of column block J+1 with this panel use a row another rank computed and sent on the side
  // stream?  (never in the row layout: a block row never changes hands — the panel stream then runs ahead of the side
  // transfers)
  std::vector<uint8_t> next_needs_side;
};

struct DistPlan {
  OwnMap map;
  uint32_t nblk = 0, nb = 0;
  std::vector<uint32_t> tiles;
  std::vector<DistPanel> panels;
  std::vector<DistMsg> msgs;
  std::vector<uint8_t> needs;   // [n][T]: rank q multiplies rows of class a
  bool need(uint32_t q, uint32_t a) const { return needs[(size_t)q * map.T + a] != 0; }
};

// nzL: nblk x nblk bytes, lower pattern of the factor (row-major, nz[i * nblk + k]); nullptr = dense.
// self_messages: single-rank self test — the one rank sends its rows to itself (exercises every code path).
inline DistPlan build_dist_plan(uint32_t nblk, const OwnMap& map, const uint8_t* nzL, bool self_messages = false) {
  DistPlan p;
  p.map = map;
  p.nblk = nblk;
  const uint32_t G = map.G, T = map.T, n = std::max(map.n, 1u);
  p.nb = (nblk + G - 1) / G;
  p.needs.assign((size_t)n * T, 0);
  for (uint32_t a = 0; a < T; ++a)
    for (uint32_t b = 0; b < T; ++b) {
      const uint32_t r = n > 1 ? map.tbl[a][b] : 0;
      p.needs[(size_t)r * T + a] = 1;   // row operand of a tile it owns
      p.needs[(size_t)r * T + b] = 1;   // column operand
    }
  p.panels.resize(p.nb);
  std::vector<std::vector<uint32_t>> own_u(n), own_r(n);
  for (uint32_t J = 0; J < p.nb; ++J) {
    DistPanel& pn = p.panels[J];
    pn.c0 = J * G;
    pn.c1 = std::min(pn.c0 + G, nblk);
    pn.diag_owner = n > 1 ? map.tbl[J % T][J % T] : 0;
    for (uint32_t r = 0; r < n; ++r) { own_u[r].clear(); own_r[r].clear(); }
    for (uint32_t i = pn.c1; i < nblk; ++i) {
      bool on = nzL == nullptr;
      for (uint32_t kb = pn.c0; kb < pn.c1 && !on; ++kb) on = nzL[(size_t)i * nblk + kb] != 0;
      if (!on) continue;
      const uint32_t r = n > 1 ? map.tbl[(i / G) % T][J % T] : 0;
      (i / G == J + 1 ? own_u[r] : own_r[r]).push_back(i);
    }
    pn.next_needs_side.assign(n, 0);
    for (uint32_t i = std::min(pn.c1 + G, nblk); i < nblk; ++i) {
      if (n <= 1) break;
      const uint32_t upd = map.tbl[(i / G) % T][(J + 1) % T], src = map.tbl[(i / G) % T][J % T];
      if (upd != src) pn.next_needs_side[upd] = 1;
    }
    pn.own_u_first.assign(n, 0); pn.own_u_count.assign(n, 0);
    pn.own_r_first.assign(n, 0); pn.own_r_count.assign(n, 0);
    for (uint32_t r = 0; r < n; ++r) {
      pn.own_u_first[r] = (uint32_t)p.tiles.size(); pn.own_u_count[r] = (uint32_t)own_u[r].size();
      p.tiles.insert(p.tiles.end(), own_u[r].begin(), own_u[r].end());
      pn.own_r_first[r] = (uint32_t)p.tiles.size(); pn.own_r_count[r] = (uint32_t)own_r[r].size();
      p.tiles.insert(p.tiles.end(), own_r[r].begin(), own_r[r].end());
    }
    // messages: the tiles of a sender grouped by the set of ranks that need their class
    for (int urgent = 1; urgent >= 0; --urgent)
      for (uint32_t s = 0; s < n; ++s) {
        const std::vector<uint32_t>& mine = urgent ? own_u[s] : own_r[s];
        if (mine.empty()) continue;
        std::map<std::vector<uint32_t>, std::vector<uint32_t>> groups;  // receivers -> tiles
        for (uint32_t i : mine) {
          const uint32_t a = (i / G) % T;
          std::vector<uint32_t> dst;
          for (uint32_t q = 0; q < n; ++q)
            if ((q != s || self_messages) && p.need(q, a)) dst.push_back(q);
          if (!dst.empty()) groups[dst].push_back(i);
        }
        for (auto& g : groups) {
          DistMsg m;
          m.panel = J; m.src = s; m.urgent = urgent != 0;
          m.first = (uint32_t)p.tiles.size(); m.count = (uint32_t)g.second.size();
          p.tiles.insert(p.tiles.end(), g.second.begin(), g.second.end());
          m.dst = g.first;
          pn.msgs.push_back((uint32_t)p.msgs.size());
          p.msgs.push_back(std::move(m));
        }
      }
  }
  return p;
}

// doubles of the square message of a panel of w tile columns: (w*64 + 1) x (w*64) factor entries (square +
// rhs row), the pivot signs, the per-tile-column sign flags, the factor packets (NOPV = 40 vectors of 64)
inline size_t dist_square_doubles(uint32_t w_tiles) {
  const size_t w = (size_t)w_tiles * 64;
  return (w + 1) * w + w + w_tiles + (size_t)w_tiles * 40 * 64;
}

struct DistPlanStats {
  double factor_bytes;            // all of L below the squares + the squares (what the 1-D panel broadcast moves)
  double chain_recv_max, chain_recv_total;   // per-rank maximum / sum over ranks, bytes per factorisation
  double side_recv_max, side_recv_total;
  double chain_sent_total, side_sent_total;  // every (message, receiver) pair once
  double recv_max;                           // chain + side of the busiest receiver
  double backward_allreduce_bytes;           // nb all-reduces of one panel width
  uint32_t messages_chain, messages_side, panels, ranks, classes;
};

inline DistPlanStats dist_plan_stats(const DistPlan& p) {
  DistPlanStats s = {};
  const uint32_t n = std::max(p.map.n, 1u);
  std::vector<double> chain(n, 0.0), side(n, 0.0);
  s.panels = p.nb; s.ranks = n; s.classes = p.map.T;
  for (uint32_t J = 0; J < p.nb; ++J) {
    const DistPanel& pn = p.panels[J];
    const uint32_t wt = pn.c1 - pn.c0;
    const double sq = 8.0 * (double)dist_square_doubles(wt);
    s.factor_bytes += sq;
    for (uint32_t r = 0; r < n; ++r) {
      if (r != pn.diag_owner) { chain[r] += sq; s.chain_sent_total += sq; }
      s.factor_bytes += 8.0 * 64.0 * 64.0 * wt * (double)(pn.own_u_count[r] + pn.own_r_count[r]);
    }
    s.backward_allreduce_bytes += 8.0 * 64.0 * wt;
    for (uint32_t mi : pn.msgs) {
      const DistMsg& m = p.msgs[mi];
      const double b = 8.0 * 64.0 * 64.0 * wt * (double)m.count;
      for (uint32_t q : m.dst) {
        if (q == m.src) continue;
        (m.urgent ? chain : side)[q] += b;
        (m.urgent ? s.chain_sent_total : s.side_sent_total) += b;
      }
      (m.urgent ? s.messages_chain : s.messages_side) += 1;
    }
  }
  for (uint32_t r = 0; r < n; ++r) {
    s.chain_recv_max = std::max(s.chain_recv_max, chain[r]); s.chain_recv_total += chain[r];
    s.side_recv_max = std::max(s.side_recv_max, side[r]); s.side_recv_total += side[r];
    s.recv_max = std::max(s.recv_max, chain[r] + side[r]);
  }
  return s;
}

// ---- the derived tables: everything dist_solve.hip uploads or sizes a buffer by ------------------------------------
// The enumeration orders are part of the result: they fix the order of the transfers and of the sums.
static const uint32_t kDistTile = 64;                    // NB of the kernels
struct DistPair { uint32_t bi, bc; };                    // as uint2 on the device
struct DistRect { uint32_t row, col, width, off; };      // as uint4: row tile, first column (doubles), columns, staging offset

// Block pairs (bi >= bc) the plan's rank owns, by block column then block row; pair_first[J] = first pair with
// bc >= J + 2 (what the bulk update of panel J touches).
struct DistOwnedPairs {
  std::vector<DistPair> pairs;
  std::vector<uint32_t> pair_first;   // [nb + 1]
};
inline DistOwnedPairs dist_owned_pairs(const DistPlan& pl) {
  const OwnMap& map = pl.map;
  DistOwnedPairs o;
  o.pair_first.assign(pl.nb + 1, 0);
  for (uint32_t bc = 0; bc < pl.nb; ++bc) {
    if (bc >= 2) o.pair_first[bc - 2] = (uint32_t)o.pairs.size();
    for (uint32_t bi = bc; bi < pl.nb; ++bi)
      if (map.n <= 1 || map.tbl[bi % map.T][bc % map.T] == map.rank) o.pairs.push_back({bi, bc});
  }
  for (uint32_t J = (pl.nb >= 2 ? pl.nb - 2 : 0); J <= pl.nb; ++J) o.pair_first[J] = (uint32_t)o.pairs.size();
  return o;
}

// Row list of every square: per panel its tiles, then the rhs row (row lists of the chain kernels).
inline std::vector<uint32_t> dist_square_rows(const DistPlan& pl) {
  std::vector<uint32_t> h;
  for (const DistPanel& pn : pl.panels) {
    for (uint32_t t = pn.c0; t < pn.c1; ++t) h.push_back(t);
    h.push_back(pl.nblk);
  }
  return h;
}

// Dense reduce-scatter of S.  Chunk of destination rank r: for every panel p, the row tiles of that panel whose
// block r owns and that hold a tile of nzS in it (nblk x nblk bytes; null: all of them) — rows[off[p N + r] ..
// off[p N + r + 1]), at chunk_off[p N + r] doubles into the chunk, panels in order.  chunk: the longest chunk, padded
// to a multiple of 64 doubles.
struct DistDenseRows {
  std::vector<uint32_t> rows, off;    // off: [npanels N + 1]
  std::vector<size_t> chunk_off;      // [npanels N]
  size_t chunk = 0;
};
inline DistDenseRows dist_dense_scatter_rows(const DistPlan& pl, const uint8_t* nzS) {
  const uint32_t nblk = pl.nblk, npanels = pl.nb, N = std::max(pl.map.n, 1u);
  DistDenseRows d;
  d.off.assign((size_t)npanels * N + 1, 0);
  d.chunk_off.assign((size_t)npanels * N, 0);
  std::vector<size_t> used(N, 0);
  for (uint32_t p = 0; p < npanels; ++p) {
    const uint32_t J = pl.panels[p].c0, Jend = pl.panels[p].c1;
    for (uint32_t r = 0; r < N; ++r) {
      OwnMap m = pl.map;
      m.rank = r;
      const size_t k = (size_t)p * N + r, before = d.rows.size();
      for (uint32_t i = J; i < nblk; ++i) {
        if (!own_tile(m, i, J, nblk)) continue;
        bool on = !nzS || i < Jend;
        for (uint32_t kb = J; kb < Jend && !on; ++kb) on = nzS[(size_t)i * nblk + kb] != 0;
        if (on) d.rows.push_back(i);
      }
      d.off[k + 1] = (uint32_t)d.rows.size();
      d.chunk_off[k] = used[r];
      used[r] += (d.rows.size() - before) * kDistTile * (size_t)(Jend - J) * kDistTile;
    }
  }
  for (size_t u : used) d.chunk = std::max(d.chunk, u);
  d.chunk = (d.chunk + 63) / 64 * 64;
  return d;
}

// Sparse exchange of S.  `all`: the local lower tile patterns of all ranks, bit i nblk + k of the `words` 64-bit words
// of rank s (dist_pack_pattern).  A rank sends a (row tile x panel) rectangle to its owner only if its own pattern
// has a tile in it.  send: the rectangles this rank sends, by destination (send_first[peer] .. send_first[peer + 1]),
// then panel, then row tile; recv: those it receives, by source, in the same order — the list a sends to b IS the
// list b receives from a.  *_off[peer]: where the peer's rectangles start in the staging half, in doubles (what the
// rectangles' 32-bit offsets count too: refused when a half exceeds `limit` doubles).
struct DistSparseRects {
  std::vector<DistRect> send, recv;
  std::vector<uint32_t> send_first, recv_first;   // [N + 1]
  std::vector<size_t> send_off, recv_off;         // [N + 1]
  std::string refused;
};
inline void dist_pack_pattern(const uint8_t* tile_nz, uint32_t nblk, unsigned long long* bits) {
  for (uint32_t i = 0; i < nblk; ++i)
    for (uint32_t k = 0; k <= i; ++k)
      if (tile_nz[(size_t)i * nblk + k]) {
        const size_t b = (size_t)i * nblk + k;
        bits[b >> 6] |= 1ull << (b & 63);
      }
}
inline size_t dist_pattern_words(uint32_t nblk) { return ((size_t)nblk * nblk + 63) / 64; }
inline DistSparseRects dist_sparse_rects(const DistPlan& pl, uint32_t rank, const unsigned long long* all, size_t words,
                                         uint64_t limit = 0xffffffffull) {
  const uint32_t nblk = pl.nblk, N = std::max(pl.map.n, 1u), NB = kDistTile;
  auto has = [&](uint32_t s_, uint32_t i, uint32_t c0, uint32_t c1) {
    for (uint32_t kb = c0; kb < c1 && kb <= i; ++kb) {
      const size_t b = (size_t)i * nblk + kb;
      if (all[(size_t)s_ * words + (b >> 6)] >> (b & 63) & 1ull) return true;
    }
    return false;
  };
  DistSparseRects t;
  t.send_first.assign(N + 1, 0); t.recv_first.assign(N + 1, 0);
  t.send_off.assign(N + 1, 0); t.recv_off.assign(N + 1, 0);
  size_t soff = 0, roff = 0;
  bool too_big = false;
  auto add = [&](std::vector<DistRect>& list, size_t& off, uint32_t i, uint32_t c0, uint32_t w) {
    too_big |= off + (size_t)NB * w > limit;
    list.push_back({i, c0 * NB, w, (uint32_t)off});
    off += (size_t)NB * w;
  };
  for (uint32_t peer = 0; peer < N; ++peer) {
    t.send_first[peer] = (uint32_t)t.send.size(); t.recv_first[peer] = (uint32_t)t.recv.size();
    t.send_off[peer] = soff; t.recv_off[peer] = roff;
    if (peer == rank) continue;
    OwnMap mp = pl.map, mr = pl.map;
    mp.rank = peer; mr.rank = rank;
    for (uint32_t p = 0; p < pl.nb; ++p) {
      const uint32_t c0 = pl.panels[p].c0, c1 = pl.panels[p].c1, w = (c1 - c0) * NB;
      for (uint32_t i = c0; i < nblk; ++i) {
        if (own_tile(mp, i, c0, nblk) && has(rank, i, c0, c1)) add(t.send, soff, i, c0, w);   // mine -> peer
        if (own_tile(mr, i, c0, nblk) && has(peer, i, c0, c1)) add(t.recv, roff, i, c0, w);   // peer -> me
      }
    }
  }
  t.send_first[N] = (uint32_t)t.send.size(); t.recv_first[N] = (uint32_t)t.recv.size();
  t.send_off[N] = soff; t.recv_off[N] = roff;
  if (too_big) t.refused = "sparse exchange of S: more than 2^32 doubles to one side (use BA_HIP_DENSE_SCATTER=1)";
  return t;
}

// Which tiles of the factor's pattern nzL a rank's assembly has to write when S is exchanged sparsely: the tiles it
// OWNS (they receive the other shards' rectangles and the factorisation's updates: they must start from its own
// partial or from zero) and the tiles of every rectangle it SENDS, i.e. where its local pattern tile_nz has a tile (a
// rectangle travels whole: tiles of it that the shard does not touch must be zeros, not last iteration's leftovers).
// Every other tile is neither read nor sent by this rank.  nblk x nblk bytes, lower triangle.
inline std::vector<uint8_t> dist_assembly_need(const DistPlan& pl, uint32_t rank, const uint8_t* tile_nz, const uint8_t* nzL) {
  const uint32_t nt = pl.nblk;
  OwnMap me = pl.map;
  me.rank = rank;
  std::vector<uint8_t> need((size_t)nt * nt, 0);
  for (uint32_t p = 0; p < pl.nb; ++p) {
    const uint32_t c0 = pl.panels[p].c0, c1 = pl.panels[p].c1;
    for (uint32_t i = c0; i < nt; ++i) {
      bool touch = own_tile(me, i, c0, nt);
      for (uint32_t kb = c0; kb < c1 && kb <= i && !touch; ++kb) touch = tile_nz[(size_t)i * nt + kb] != 0;
      if (!touch) continue;
      for (uint32_t kb = c0; kb < c1 && kb <= i; ++kb)
        if (nzL[(size_t)i * nt + kb]) need[(size_t)i * nt + kb] = 1;
    }
  }
  return need;
}

// Doubles of the point-to-point staging buffers of `rank`: the urgent / side messages it sends / receives in its
// busiest panel (at least 1).
struct DistStagingCaps { size_t usend = 1, urecv = 1, ssend = 1, srecv = 1; };
inline DistStagingCaps dist_staging_caps(const DistPlan& pl, uint32_t rank) {
  DistStagingCaps c;
  for (const DistPanel& pn : pl.panels) {
    size_t us = 0, ur = 0, ss = 0, sr = 0;
    const size_t w = (size_t)(pn.c1 - pn.c0) * kDistTile;
    for (uint32_t mi : pn.msgs) {
      const DistMsg& m = pl.msgs[mi];
      const size_t cnt = (size_t)m.count * kDistTile * w;
      const bool recv = std::find(m.dst.begin(), m.dst.end(), rank) != m.dst.end();
      if (m.src == rank) (m.urgent ? us : ss) += cnt;
      if (recv) (m.urgent ? ur : sr) += cnt;
    }
    c.usend = std::max(c.usend, us); c.urecv = std::max(c.urecv, ur);
    c.ssend = std::max(c.ssend, ss); c.srecv = std::max(c.srecv, sr);
  }
  return c;
}

// Tile products one bulk update forms on `rank` (flop accounting of the profiled launches): per tile column kb of
// the panel [c0, c1) the tiles (i, c), i >= c >= first, the rank owns and whose two operand tiles (i, kb), (c, kb)
// are in nzL (null: dense), plus the rhs row's; per row class a suffix count of the nonzero tiles of the column.
// Summed over the ranks — or with own_map_single() — that is sum over kb of m (m + 1) / 2 + m, m = the nonzero
// tiles of column kb from row `first` on.
inline double bulk_update_tile_products(const OwnMap& own, uint32_t rank, uint32_t nblk, uint32_t first, uint32_t c0,
                                        uint32_t c1, const uint8_t* nzL) {
  double tiles = 0.0;
  std::vector<double> suffix((size_t)own.T * (nblk + 1));
  for (uint32_t kb = c0; kb < c1; ++kb) {
    for (uint32_t a = 0; a < own.T; ++a) suffix[(size_t)a * (nblk + 1) + nblk] = 0.0;
    for (uint32_t r = nblk; r-- > first;)
      for (uint32_t a = 0; a < own.T; ++a)
        suffix[(size_t)a * (nblk + 1) + r] = suffix[(size_t)a * (nblk + 1) + r + 1] +
            (((r / own.G) % own.T == a && (!nzL || nzL[(size_t)r * nblk + kb])) ? 1.0 : 0.0);
    for (uint32_t c = first; c < nblk; ++c) {
      if (nzL && !nzL[(size_t)c * nblk + kb]) continue;
      const uint32_t cc = (c / own.G) % own.T;
      for (uint32_t a = 0; a < own.T; ++a)
        if (own.n <= 1 || own.tbl[a][cc] == rank) tiles += suffix[(size_t)a * (nblk + 1) + c];
      if (own.n <= 1 || own.tbl[cc][cc] == rank) tiles += 1.0;  // the rhs row
    }
  }
  return tiles;
}

// What the engine keeps per plan: the tables of the plan alone, and the two that need a further input (the S pattern /
// the all-gathered local patterns), built by the first exchange that needs them.  A new plan replaces all of them.
struct DistTables {
  DistOwnedPairs own;
  std::vector<uint32_t> square_rows;
  DistStagingCaps caps;
  bool have_dense = false, have_sparse = false;
  DistDenseRows dense;
  DistSparseRects sparse;
  DistTables() = default;
  explicit DistTables(const DistPlan& pl)
      : own(dist_owned_pairs(pl)), square_rows(dist_square_rows(pl)), caps(dist_staging_caps(pl, pl.map.rank)) {}
};

}  // namespace bae
