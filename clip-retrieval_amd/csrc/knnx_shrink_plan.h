// knnx_shrink_plan.h -- the integer arithmetic of shrinking a built IVF index (knnx_ivf_remove_ids; include/knnx.h, "Shrinking a built
// index").  No device code in here: what the kernels of knn_shrink_kernels.hip and the host of knnx_shrink.hip share, written
// so that a host-only program can drive every piece against a plain sequential reference (tools/shrink_plan_check.cpp).
//
// Ids are positional: the row with id id_base + o is row o of the corpus.  Removing a set of ids renumbers the survivors densely in id
// order (new id = id_base + the number of surviving ids below it) and lays their lists down again by the rule of knnx_ivf_begin
// (grow_layout in knnx_grow_plan.h); inside a list the survivors keep their order.  The steps, each stated here once:
//   * rank: the id space is cut into blocks of SHRINK_BLOCK ids; a block's survivors are counted, the counts are scanned on the host
//     (shrink_block_scan, accumulated in int64), and a survivor's new id is its block's offset + its rank inside the block;
//   * mask: a source tile (32 arena rows) has a 32-bit survivor mask, bit b = the row at 32 t + b holds an id that survives;
//   * position: the survivor at bit b of tile t goes to destination arena row dst0[t] + shrink_pos(mask, b), so the survivors of one
//     source tile are ONE contiguous run of the destination; dst0[t] = 32 * tile0_new[l] + the survivors in the tiles of list l before t
//     (shrink_list_scan gives the second term and the new list sizes, shrink_dst0 adds the first once the host has the new layout);
//   * checks: the new sizes must add up to the survivors the id scan counted (two independent computations), and the padded rows of the
//     new arena must stay below 2^32 (they cannot exceed the old arena's; asserted all the same).
#pragma once

#include <stdint.h>
#include <algorithm>
#include <vector>

#include "knnx_grow_plan.h"

// the kernels compile the two one-line rules below for the device as well: their file defines this before it includes the header
#ifndef KNNX_SHRINK_FN
#define KNNX_SHRINK_FN inline
#endif

namespace knnx {

constexpr int64_t SHRINK_BLOCK = 1024;  // ids of one block of the rank scan (one wave: 64 lanes x 16 flag bytes)

enum { SHRINK_OK = 0, SHRINK_E_ROWS = 1, SHRINK_E_COUNT = 2, SHRINK_E_LAYOUT = 3 };

// survivors of a tile in front of bit b of its mask (b < 32)
KNNX_SHRINK_FN unsigned shrink_pos(uint32_t mask, unsigned b) { return (unsigned)__builtin_popcount(mask & ((1u << b) - 1u)); }
// id - id_lo as an index into [0, n), or n where the id names no row (-1, below id_lo, at or above id_lo + n; no signed overflow)
KNNX_SHRINK_FN uint64_t shrink_index(int64_t id, int64_t id_lo, int64_t n) {
  const uint64_t o = (uint64_t)id - (uint64_t)id_lo;
  return id >= id_lo && o < (uint64_t)n ? o : (uint64_t)n;
}

inline int64_t shrink_blocks(int64_t n) { return (n + SHRINK_BLOCK - 1) / SHRINK_BLOCK; }

// survivors of every block of ids: sums [shrink_blocks(n)]
inline void shrink_block_sums(const uint8_t* dead, int64_t n, std::vector<uint32_t>& sums) {
  sums.assign((size_t)shrink_blocks(n), 0u);
  for (int64_t i = 0; i < n; ++i) sums[(size_t)(i / SHRINK_BLOCK)] += dead[i] ? 0u : 1u;
}

// exclusive scan of the block sums in int64 -> off [nblk] (32-bit: a rank is an index into inv), total survivors.  SHRINK_E_COUNT when a
// block claims more than SHRINK_BLOCK survivors or the total exceeds n; off is left in an unspecified state then.
inline int shrink_block_scan(const uint32_t* sums, int64_t nblk, int64_t n, std::vector<uint32_t>& off, int64_t& total) {
  off.assign((size_t)std::max<int64_t>(nblk, 0), 0u);
  total = 0;
  for (int64_t b = 0; b < nblk; ++b) {
    if ((int64_t)sums[b] > SHRINK_BLOCK) return SHRINK_E_COUNT;
    if (total > GROW_MAX_PROWS) return SHRINK_E_ROWS;
    off[(size_t)b] = (uint32_t)total;
    total += (int64_t)sums[b];
  }
  return total > n ? SHRINK_E_COUNT : SHRINK_OK;
}

// the new id (without id_base) of every id: rank [n]; the entry of a dead id is the rank its successor would get
inline void shrink_ranks(const uint8_t* dead, int64_t n, const std::vector<uint32_t>& off, std::vector<uint32_t>& rank) {
  rank.assign((size_t)n, 0u);
  for (int64_t b = 0; b * SHRINK_BLOCK < n; ++b) {
    uint32_t run = off[(size_t)b];
    for (int64_t i = b * SHRINK_BLOCK; i < std::min(n, (b + 1) * SHRINK_BLOCK); ++i) {
      rank[(size_t)i] = run;
      run += dead[i] ? 0u : 1u;
    }
  }
}

// the survivor mask of every source tile: tmask [prow / 32] from idmap [prow] (-1 on pad rows) and dead [n]
inline void shrink_masks(const int64_t* idmap, int64_t prow, int64_t id_lo, int64_t n, const uint8_t* dead, std::vector<uint32_t>& tmask) {
  tmask.assign((size_t)(prow / 32), 0u);
  for (int64_t r = 0; r < prow; ++r) {
    const uint64_t o = shrink_index(idmap[r], id_lo, n);
    if (o < (uint64_t)n && !dead[o]) tmask[(size_t)(r >> 5)] |= 1u << (r & 31);
  }
}

// per list: tpos[t] = survivors in the tiles of the list in front of tile t (tiles of no list keep 0), size_new[l] = survivors of list l
inline void shrink_list_scan(int64_t nlist, const unsigned* tile0, const unsigned* ntile, const std::vector<uint32_t>& tmask,
                             std::vector<uint32_t>& tpos, std::vector<int64_t>& size_new) {
  tpos.assign(tmask.size(), 0u);
  size_new.assign((size_t)std::max<int64_t>(nlist, 0), 0);
  for (int64_t l = 0; l < nlist; ++l) {
    uint32_t run = 0;
    for (unsigned t = tile0[l]; t < tile0[l] + ntile[l]; ++t) {
      tpos[t] = run;
      run += (uint32_t)__builtin_popcount(tmask[t]);
    }
    size_new[(size_t)l] = run;
  }
}

// tpos -> dst0 in place: the destination arena row of every source tile's first survivor
inline void shrink_dst0(int64_t nlist, const unsigned* tile0_old, const unsigned* ntile_old, const unsigned* tile0_new, std::vector<uint32_t>& tpos) {
  for (int64_t l = 0; l < nlist; ++l)
    for (unsigned t = tile0_old[l]; t < tile0_old[l] + ntile_old[l]; ++t) tpos[t] += 32u * tile0_new[l];
}

// the new layout from the new sizes, and the two checks: SHRINK_E_COUNT when the sizes do not add up to the survivors of the id scan,
// SHRINK_E_ROWS past 2^32 padded rows, SHRINK_E_LAYOUT when a list grew or the new arena is larger than the old one
inline int shrink_layout(int64_t nlist, const unsigned* size_old, const int64_t* size_new, int64_t survivors, int64_t old_prow,
                         std::vector<unsigned>& tile0, std::vector<unsigned>& ntile, std::vector<unsigned>& size, int64_t& tiles, int64_t& prow) {
  for (int64_t l = 0; l < nlist; ++l)
    if (size_new[l] < 0 || size_new[l] > (int64_t)size_old[l]) return SHRINK_E_LAYOUT;
  int64_t rows = 0;
  const int r = grow_layout(nlist, size_new, tile0, ntile, size, rows, tiles, prow);
  if (r == GROW_E_ROWS) return SHRINK_E_ROWS;
  if (r) return SHRINK_E_LAYOUT;
  if (rows != survivors) return SHRINK_E_COUNT;
  if (prow > old_prow || prow > GROW_MAX_PROWS) return SHRINK_E_LAYOUT;
  return SHRINK_OK;
}

// ---- the reference: one plain walk over the old arena, list by list, row by row
struct ShrinkRef {
  std::vector<unsigned> tile0, ntile, size;  // the new layout
  int64_t rows = 0, tiles = 0, prow = 0;
  std::vector<int64_t> dest;                 // [old prow] destination arena row of every source row, -1 where it has none
  std::vector<int64_t> idmap;                // [prow] new id of every destination row, -1 on pad rows
  std::vector<uint32_t> inv;                 // [rows] new id - id_lo -> destination row
};

inline int shrink_reference(int64_t nlist, const unsigned* size_old, const int64_t* idmap_old, int64_t id_lo, int64_t n, const uint8_t* dead,
                            ShrinkRef& R) {
  R = ShrinkRef();
  std::vector<int64_t> newid((size_t)n, -1), size_new((size_t)nlist, 0);
  int64_t next = 0;
  for (int64_t i = 0; i < n; ++i)
    if (!dead[i]) newid[(size_t)i] = id_lo + next++;
  int64_t t0 = 0;
  std::vector<int64_t> first((size_t)nlist, 0);
  for (int64_t l = 0; l < nlist; ++l) {
    first[(size_t)l] = t0 * 32;
    for (int64_t j = 0; j < (int64_t)size_old[l]; ++j) {
      const int64_t id = idmap_old[t0 * 32 + j];
      if (id < id_lo || id - id_lo >= n) return SHRINK_E_LAYOUT;
      if (!dead[id - id_lo]) size_new[(size_t)l]++;
    }
    t0 += ((int64_t)size_old[l] + 31) / 32;
  }
  if (grow_layout(nlist, size_new.data(), R.tile0, R.ntile, R.size, R.rows, R.tiles, R.prow)) return SHRINK_E_LAYOUT;
  R.dest.assign((size_t)std::max<int64_t>(t0 * 32, 32), -1);
  R.idmap.assign((size_t)R.prow, -1);
  R.inv.assign((size_t)R.rows, 0u);
  for (int64_t l = 0; l < nlist; ++l) {
    int64_t out = (int64_t)R.tile0[(size_t)l] * 32;
    for (int64_t j = 0; j < (int64_t)size_old[l]; ++j) {
      const int64_t r = first[(size_t)l] + j, o = idmap_old[r] - id_lo;
      if (dead[o]) continue;
      R.dest[(size_t)r] = out;
      R.idmap[(size_t)out] = newid[(size_t)o];
      R.inv[(size_t)(newid[(size_t)o] - id_lo)] = (uint32_t)out;
      ++out;
    }
  }
  return next == R.rows ? SHRINK_OK : SHRINK_E_COUNT;
}

}  // namespace knnx
