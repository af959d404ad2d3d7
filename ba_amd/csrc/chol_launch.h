// Host decisions of the LDL^T solve (k_chol.hip, and its distributed driver dist_solve.hip): its environment
// switches, the shapes of its launches, the layout of its work space and the key of the distributed plan (the plan
// and its tables: dist_plan.h).  Integers in, small structs out — no HIP type, so hostcheck.cpp evaluates the same
// functions on the CPU (ba_hostcheck_chol_launch, tests/test_chol_launch.py).  These are the only getenv calls of the
// solve (DESIGN.md 9.1a has the table).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace bae {

static const uint32_t kTile = 64;                        // NB of k_chol.hip
static const uint32_t kPacketStride = 40 * 64;           // doubles per factor packet: NOPV vectors of 64
static const uint32_t kKin = 4;                          // tile columns of a sub-panel of the chain (8 when left-looking)

struct CholSwitches {
  // --- read once per process (A/B switches: tests set them for a child process)
  bool no128 = false;             // BA_HIP_NO128: no 128x128 blocks anywhere
  bool no_lookahead = false;      // BA_HIP_NO_LOOKAHEAD: bulk updates on the chain stream
  bool bulk_full = false;         // BA_HIP_BULK_FULL: never the capped bulk kernel
  bool dense = false;             // BA_HIP_DENSE: no tile pattern
  bool no_dist_solve = false;     // BA_HIP_NO_DIST_SOLVE
  uint32_t sbl = 3;               // BA_HIP_SBL: log2 of the super-block edge of the 64-tile bulk kernel
  // BA_HIP_BULK_FULL_M = v, two readings (both 128 when unset):
  uint32_t rect_min_rows = 128;   //   max(16, v): tile rows below the next panel from which its rectangle goes to k_update128
  uint32_t bulk_full_m = 128;     //   v: trailing tile rows from which the bulk update runs uncapped
  bool c_rmw = false;             // BA_HIP_C_RMW: k_update128 reads, subtracts and stores C (default: memory-side FP64 adds)
  bool bulk_grid = false;         // BA_HIP_BULK_GRID: the bulk update covers the whole block triangle (default: bulk_lists.h)
  // --- read on every call (tests vary them inside one process)
  uint32_t kout = 4;              // BA_HIP_KOUT: tiles per outer panel; 0 / unset: by nblk
  uint32_t left_min_tiles = 512;  // BA_HIP_LEFT_MIN_TILES: left-looking sub-panels from this many tiles on
  bool square = false;            // BA_HIP_SQUARE != 0 and nblk < 512: k_square / k_rowpanel
  uint32_t sq_w = kKin;           // BA_HIP_SQ_W: width of their squares, 1..4
  const char* dist_layout = nullptr;  // BA_HIP_DIST_LAYOUT
  bool dense_scatter = false;     // BA_HIP_DENSE_SCATTER
  const char* trace_file = nullptr;   // BA_HIP_TRACE_FILE (BAE_TIME128 builds)
  bool lists_report = false;      // BA_HIP_BULK_LISTS_REPORT: one line on stderr per build of the bulk block lists
};

// The parsing, on the variables' values (null = unset).
inline uint32_t parse_kout(const char* v, uint32_t nblk) {
  const uint32_t k = v ? (uint32_t)atoi(v) : 0;
  return k ? k : (nblk >= 400 ? 16u : nblk >= 256 ? 8u : 4u);  // measured at 94 / 282 / 469 / 938 tiles
}
inline void parse_process_switches(CholSwitches* sw, const char* no128, const char* no_lookahead, const char* bulk_full,
                                   const char* dense, const char* no_dist_solve, const char* sbl,
                                   const char* bulk_full_m, const char* c_rmw = nullptr,
                                   const char* bulk_grid = nullptr) {
  sw->no128 = no128 != nullptr;
  sw->no_lookahead = no_lookahead != nullptr;
  sw->bulk_full = bulk_full != nullptr;
  sw->dense = dense != nullptr;
  sw->no_dist_solve = no_dist_solve != nullptr;
  sw->sbl = sbl ? (uint32_t)atoi(sbl) : 3u;
  sw->rect_min_rows = bulk_full_m ? (uint32_t)std::max(16, atoi(bulk_full_m)) : 128u;
  sw->bulk_full_m = bulk_full_m ? (uint32_t)atoi(bulk_full_m) : 128u;
  sw->c_rmw = c_rmw != nullptr;
  sw->bulk_grid = bulk_grid != nullptr;
}
inline void parse_call_switches(CholSwitches* sw, uint32_t nblk, const char* kout, const char* left_min_tiles,
                                const char* square, const char* sq_w, const char* dist_layout,
                                const char* dense_scatter, const char* trace_file,
                                const char* lists_report = nullptr) {
  sw->kout = parse_kout(kout, nblk);
  sw->left_min_tiles = left_min_tiles ? (uint32_t)std::max(1, atoi(left_min_tiles)) : 512u;
  sw->square = nblk < 512 && square && atoi(square) != 0;
  sw->sq_w = sq_w ? std::min(4u, std::max(1u, (uint32_t)atoi(sq_w))) : kKin;
  sw->dist_layout = dist_layout;
  sw->dense_scatter = dense_scatter != nullptr;
  sw->trace_file = trace_file;
  sw->lists_report = lists_report != nullptr;
}

inline const CholSwitches& chol_process_switches() {
  static const CholSwitches once = [] {
    CholSwitches sw;
    parse_process_switches(&sw, getenv("BA_HIP_NO128"), getenv("BA_HIP_NO_LOOKAHEAD"), getenv("BA_HIP_BULK_FULL"),
                           getenv("BA_HIP_DENSE"), getenv("BA_HIP_NO_DIST_SOLVE"), getenv("BA_HIP_SBL"),
                           getenv("BA_HIP_BULK_FULL_M"), getenv("BA_HIP_C_RMW"), getenv("BA_HIP_BULK_GRID"));
    return sw;
  }();
  return once;
}
// Every switch, for a solve of nblk tiles: the entry points of k_chol.hip / dist_solve.hip call this once and hand it down.
inline CholSwitches chol_switches(uint32_t nblk) {
  CholSwitches sw = chol_process_switches();
  parse_call_switches(&sw, nblk, getenv("BA_HIP_KOUT"), getenv("BA_HIP_LEFT_MIN_TILES"), getenv("BA_HIP_SQUARE"),
                      getenv("BA_HIP_SQ_W"), getenv("BA_HIP_DIST_LAYOUT"), getenv("BA_HIP_DENSE_SCATTER"),
                      getenv("BA_HIP_TRACE_FILE"), getenv("BA_HIP_BULK_LISTS_REPORT"));
  return sw;
}
inline uint32_t kout_from_env(uint32_t nblk) { return parse_kout(getenv("BA_HIP_KOUT"), nblk); }

// ---- launch shapes ---------------------------------------------------------------------------------------------
// Sub-panels of the serial chain.  Large systems (the chain's tile updates are bandwidth-bound there and cost the
// bulk update their full duration): sub-panels of 8, left-looking inside — every column is read and written once
// per sub-panel instead of once per earlier column.  Small systems are latency-bound on the diagonal tile:
// right-looking keeps its update shallow (K = 64).
struct ChainShape { bool left; uint32_t kin; };
inline ChainShape chain_shape(uint32_t nblk, const CholSwitches& sw) {
  const bool left = nblk >= sw.left_min_tiles;
  return {left, left ? 2 * kKin : kKin};
}

// The rectangle below the next panel — tile columns [c0, c0 + ncols), the m = nblk - c0 - ncols tile rows under
// them — as 128x128 blocks of k_update128<true>: nrow64 leading workgroups for the 64-tile leftovers (the rhs row and
// an odd last tile row; a multiple of 8 keeps the XCD phase of the blocks), then m2 x rect_cols blocks.
struct Rect128Shape { bool use128; uint32_t m2, rect_cols, nrow64, grid; };
enum RectRule { kRectSingle, kRectDist };
inline Rect128Shape rect128_shape(RectRule rule, uint32_t nblk, uint32_t c0, uint32_t ncols, uint32_t G,
                                  const CholSwitches& sw) {
  const uint32_t r0 = c0 + ncols, m = nblk - r0;
  // cholesky_solve: the rectangle is a SECOND launch on the serial chain stream, behind the k_step_update of the
  // panel's own triangle — worth it only where the chain is not the bottleneck, from rect_min_rows tile rows on.
  const bool single = r0 + sw.rect_min_rows <= nblk;
  // cholesky_solve_dist: the rectangle runs on the panel stream, INSTEAD of the 64-tile launch there, so the chain
  // argument does not apply; the floor is the 16 tile rows of the bulk 128-block launch (bulk_shape; no measurement
  // of this floor is on record).  A 128-block must lie inside one G x G ownership block (k_update128 tests the
  // ownership of its first tile only), hence G even.
  const bool dist = m >= 16 && G % 2u == 0;
  Rect128Shape r = {!sw.no128 && (rule == kRectSingle ? single : dist) && ncols % 2u == 0 && c0 % 2u == 0, 0, 0, 0, 0};
  if (!r.use128) return r;
  r.m2 = m / 2;
  r.rect_cols = ncols / 2;
  r.nrow64 = (ncols * (1 + (m & 1u)) + 7) / 8 * 8;
  r.grid = r.nrow64 + r.m2 * r.rect_cols;
  return r;
}

// Bulk trailing update of the tile rows / columns >= a_end.  Big trailing matrices: 128x128 blocks over the even
// part (k_update128, XCD-aware 4x4 super-blocks = the footprint of the 64-tile kernel's 8x8; the rhs row and an odd
// last tile row ride along as 64-tiles) — all of the triangle, or with have_pairs the npairs ownership blocks of
// this rank, or with list_len >= 0 the list_len entries (8 x the longest per-XCD sub-list, sentinels included) of
// the launch's list of non-empty blocks (bulk_lists.h); otherwise the 64-tile kernel over its 2^sbl super-blocks,
// capped (`full` = false) to leave the chain room.
enum BulkKernel { kBulkU128, kBulkU128List, kBulkU2Full, kBulkU2Capped, kBulkU128Blocks };
struct BulkShape { BulkKernel kernel; uint32_t grid, nrow64, m2, sbl; int swzf; };
inline BulkShape bulk_shape(uint32_t nblk, uint32_t a_end, bool full, uint32_t own_n, uint32_t own_G, bool have_pairs,
                            uint32_t npairs, const CholSwitches& sw, int64_t list_len = -1) {
  const uint32_t m = nblk - a_end;
  if (full && !sw.no128 && m >= 16 && (a_end % 2u) == 0 && (own_n <= 1 || own_G % 2u == 0)) {
    const uint32_t m2 = m / 2, sbl2 = 2, sbe2 = 1u << sbl2;
    const uint32_t nsr = (m2 + sbe2 - 1) / sbe2, nsb = nsr * (nsr + 1) / 2;
    const uint32_t nrow64 = (m * (1 + (m & 1u)) + 7) / 8 * 8;
    if (have_pairs && own_n > 1 && a_end % own_G == 0)
      return {kBulkU128List, nrow64 + npairs * (own_G / 2) * (own_G / 2), nrow64, m2, sbl2, 0};
    if (list_len >= 0 && own_n <= 1 && !sw.bulk_grid)
      return {kBulkU128Blocks, nrow64 + (uint32_t)list_len, nrow64, m2, sbl2, 0};
    return {kBulkU128, nrow64 + ((nsb + 7) / 8) * 8 * sbe2 * sbe2, nrow64, m2, sbl2, 0};
  }
  // 1-D XCD-aware launch over the super-blocks of the (m + 1) x m lower-triangular tile region
  const uint32_t sbe = 1u << sw.sbl;
  const uint32_t nsr = (m + 1 + sbe - 1) / sbe, nsb = nsr * (nsr + 1) / 2;
  return {full ? kBulkU2Full : kBulkU2Capped, ((nsb + 7) / 8) * 8 * sbe * sbe, 0, 0, sw.sbl, 1 | (int)(sw.sbl << 8)};
}

// ---- Engine::invdiag for nblk tiles, offsets in doubles:  pivot signs | L_JJ^-T | factor packets | colneg ---------
struct FactorWork {
  size_t dsgn, linvT, opbuf, colneg, total;
  explicit FactorWork(uint32_t nblk)
      : dsgn(0), linvT((size_t)nblk * kTile), opbuf(linvT + (size_t)nblk * kTile * kTile),
        colneg(opbuf + (size_t)nblk * kPacketStride), total(colneg + (nblk + 1) / 2) {}  // colneg: one int per tile column
};

// ---- key of the cached distributed plan and its tables (Engine::dist.key; ~0 = none) -------------------------------
// Everything ensure_dist_plan's result depends on besides nblk and the communicator: the pattern version (if the
// plan uses the pattern), the panel width, the layout and the kind of S exchange.  Layouts that cannot give a plan
// share one code: build_own_map rejects them and nothing is cached.
inline uint64_t dist_plan_key(uint64_t nzL_version, uint32_t kout, bool pat, const char* layout, bool dense_scatter) {
  static const char* const names[] = {"auto", "tri", "grid", "col", "row"};
  uint64_t lay = layout && *layout ? 5 : 0;   // unset = auto
  for (uint64_t i = 0; i < 5 && lay == 5; ++i)
    if (!strcmp(layout, names[i])) lay = i;
  return (pat ? nzL_version : 0) << 24 | (uint64_t)std::min(kout, 0xffffu) << 8 | lay << 2 |
         (dense_scatter ? 2u : 0u) | (pat ? 1u : 0u);
}

}  // namespace bae
