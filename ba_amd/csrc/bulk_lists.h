// The non-empty 128-blocks of the bulk LDL^T updates of one solve, as launch lists (k_chol.hip: cholesky_solve,
// k_update128<false, true>).  A grid launch over the whole lower triangle of 128-blocks starts a workgroup for every
// position; on a banded pattern more than half of them find C > R, R >= m2 or an empty K mask and leave, each after
// waiting for one of the two workgroup slots of a CU.  The pattern is fixed between two structure changes, so the
// blocks that do work are listed once per pattern and the launch covers the list.
// Integers and a host pattern in, plain vectors out — no HIP type, so hostcheck.cpp runs the same builder on the CPU
// (ba_hostcheck_bulk_lists, tests/test_bulk_block_lists.py).
#pragma once
#include <stdint.h>

#include <vector>

#include "chol_launch.h"

namespace bae {

// One list entry: the block's position in the launch's own coordinates (tile row a_end + 2 R, tile column
// a_end + 2 C) and its K mask (bit l: tile column J + l is active; what makes the block non-empty — the kernel forms
// it again from the pattern, the device list carries the position only).  R = kBulkSentinel: padding, the workgroup
// returns.
static const uint32_t kBulkSentinel = 0xffffffffu;
struct BulkEntry { uint32_t R, C; uint64_t mask; };

// Lists above this many bytes on the device are not built: the solve keeps the grid launch.  An entry costs 8 bytes
// there (block row, block column).  The flagship scene (938 tile columns, 973 680 entries) needs 7.8 MB, a dense
// pattern of that size 15.9 MB: 64 MiB (8.4 M entries) holds both four times over and is 0.2 % of the 29 GB of S
// there.  The lists grow with the cube of the tile count at a fixed band ratio, S with its square: a dense pattern of
// 2 344 tile columns would take 260 MB beside 180 GB of S on a device that has little else left, and keeps the grid
// launch.  A constant, not a share of the free memory: which launch runs must not depend on what else is allocated.
static const size_t kBulkListBudgetBytes = (size_t)64 << 20;
static const size_t kBulkListDeviceEntryBytes = 8;

struct BulkLaunchList {
  uint32_t a_end, J, Jend;   // the launch: tile rows / columns >= a_end, tile columns [J, Jend) of the panel
  uint32_t first, len;       // its slice of BulkLists::entries; len = 8 x the longest sub-list
  uint32_t blocks;           // entries that are no sentinels
  uint32_t xcd_blocks[8];    // ... per XCD class (list position mod 8)
};
struct BulkLists {
  bool built = false;        // false: no lists (kout > 64, or over the budget) — grid launches
  std::vector<BulkLaunchList> launches;   // in launch order; only the launches bulk_shape gives to kBulkU128
  std::vector<BulkEntry> entries;
  uint64_t total_blocks = 0;
};

// Is the bulk launch behind panel [J, Jend) of a single-GPU solve uncapped?  (cholesky_solve's rule.)
inline bool bulk_launch_full(uint32_t nblk, uint32_t a_end, const CholSwitches& sw) {
  return sw.no_lookahead || sw.bulk_full || nblk - a_end >= sw.bulk_full_m;
}

// The list of one launch, appended to out->entries.  nz: nblk x nblk bytes, lower (the factor's tile pattern).
// The kernel's rule: tile column k of [J, Jend) is active for block (R, C) when nz[i,k] | nz[i+1,k] and
// nz[c,k] | nz[c+1,k], i = a_end + 2R, c = a_end + 2C — a per-row-block mask, and the block's is the AND of two.
// Order: the 4x4 super-blocks in the triangular order of the grid launch; each non-empty one goes, whole and in its
// `within` order, to the XCD class (list position mod 8: workgroup ids are dealt round-robin over the 8 XCDs) that
// holds the fewest blocks so far, ties to the lowest; the eight sub-lists are interleaved, the shorter ones padded
// at their end with sentinels.  Least-count dealing of items of at most 16 keeps the counts within 16 of each other.
inline void build_bulk_launch_list(uint32_t nblk, uint32_t a_end, uint32_t J, uint32_t Jend, const uint8_t* nz,
                                   BulkLists* out) {
  const uint32_t m2 = (nblk - a_end) / 2, sbe = 4, nsr = (m2 + sbe - 1) / sbe;
  const uint32_t ncol = Jend - J < 64u ? Jend - J : 64u;   // the kernel's mask is one ballot: 64 tile columns
  std::vector<uint64_t> rowmask(m2, 0);
  for (uint32_t R = 0; R < m2; ++R) {
    const uint8_t* r0 = nz + (size_t)(a_end + 2 * R) * nblk + J;
    const uint8_t* r1 = r0 + nblk;
    uint64_t mk = 0;
    for (uint32_t l = 0; l < ncol; ++l)
      if (r0[l] | r1[l]) mk |= 1ull << l;
    rowmask[R] = mk;
  }
  std::vector<BulkEntry> sub[8];
  for (uint32_t sr = 0; sr < nsr; ++sr)
    for (uint32_t sc = 0; sc <= sr; ++sc) {
      BulkEntry blk[16];
      uint32_t nb = 0;
      for (uint32_t within = 0; within < sbe * sbe; ++within) {
        const uint32_t R = sr * sbe + within / sbe, C = sc * sbe + within % sbe;
        if (C > R || R >= m2) continue;
        const uint64_t mk = rowmask[R] & rowmask[C];
        if (mk) blk[nb++] = {R, C, mk};
      }
      if (!nb) continue;
      uint32_t x = 0;
      for (uint32_t y = 1; y < 8; ++y)
        if (sub[y].size() < sub[x].size()) x = y;
      sub[x].insert(sub[x].end(), blk, blk + nb);
    }
  BulkLaunchList l = {};
  l.a_end = a_end; l.J = J; l.Jend = Jend;
  l.first = (uint32_t)out->entries.size();
  size_t longest = 0;
  for (uint32_t x = 0; x < 8; ++x) {
    l.xcd_blocks[x] = (uint32_t)sub[x].size();
    l.blocks += l.xcd_blocks[x];
    if (sub[x].size() > longest) longest = sub[x].size();
  }
  l.len = (uint32_t)(8 * longest);
  const BulkEntry none = {kBulkSentinel, kBulkSentinel, 0};
  for (size_t k = 0; k < longest; ++k)
    for (uint32_t x = 0; x < 8; ++x) out->entries.push_back(k < sub[x].size() ? sub[x][k] : none);
  out->total_blocks += l.blocks;
  out->launches.push_back(l);
}

// Every bulk launch of a single-GPU solve of nblk tiles with panels of kout that bulk_shape gives to kBulkU128
// (cholesky_solve's loop).  Nothing is built (built = false) without a pattern, for panels wider than one ballot,
// or when the lists would exceed budget_bytes on the device.
inline BulkLists build_bulk_lists(uint32_t nblk, uint32_t kout, const uint8_t* nz, const CholSwitches& sw,
                                  size_t budget_bytes = kBulkListBudgetBytes) {
  BulkLists out;
  if (!nz || !kout || kout > 64u || sw.bulk_grid || sw.dense) return out;
  for (uint32_t J = 0; J < nblk; J += kout) {
    const uint32_t Jend = J + kout < nblk ? J + kout : nblk;
    if (Jend >= nblk) break;
    const uint32_t a_end = Jend + kout < nblk ? Jend + kout : nblk;
    if (a_end >= nblk) continue;
    if (bulk_shape(nblk, a_end, bulk_launch_full(nblk, a_end, sw), 1, 1, false, 0, sw).kernel != kBulkU128) continue;
    build_bulk_launch_list(nblk, a_end, J, Jend, nz, &out);
    if (out.entries.size() * kBulkListDeviceEntryBytes > budget_bytes) return BulkLists();
  }
  out.built = true;
  return out;
}

// What the cached lists of an engine depend on (Engine::bulk_lists_key): the pattern version and the inputs of the
// set of launches.
struct BulkListsKey {
  uint64_t nzL_version = ~0ull;
  uint32_t nblk = 0, kout = 0, bulk_full_m = 0;
  bool no128 = false, full_always = false;
  bool operator==(const BulkListsKey& o) const {
    return nzL_version == o.nzL_version && nblk == o.nblk && kout == o.kout && bulk_full_m == o.bulk_full_m &&
           no128 == o.no128 && full_always == o.full_always;
  }
};
inline BulkListsKey bulk_lists_key(uint64_t nzL_version, uint32_t nblk, const CholSwitches& sw) {
  BulkListsKey k;
  k.nzL_version = nzL_version; k.nblk = nblk; k.kout = sw.kout; k.bulk_full_m = sw.bulk_full_m;
  k.no128 = sw.no128; k.full_always = sw.no_lookahead || sw.bulk_full;
  return k;
}

}  // namespace bae
