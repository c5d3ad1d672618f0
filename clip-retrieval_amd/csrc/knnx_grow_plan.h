// knnx_grow_plan.h -- the host arithmetic of growing a built IVF index (knnx_ivf_append* / knnx_ivf_merge_from; include/knnx.h, "Growing
// a built index").  No device code in here: plain integer arithmetic on list sizes, so that a host-only program can drive it
// (tools/grow_plan_check.cpp).
//
// The arena of a built index is dense: list l holds size[l] rows at arena rows 32 * tile0[l] + j, tile0 = the exclusive prefix sum of
// ntile[l] = ceil(size[l] / 32).  When lists grow every later list moves, so growing is a layout-to-layout move into a new arena.  The plan:
//   * the new layout, the rule of knnx_ivf_begin applied to size_old[l] + extra[l];
//   * src_tile [max(new tiles, 1)]: the OLD tile every NEW tile is copied from, GROW_NO_TILE where there is none (tiles a list gained,
//     and the one tile of an empty arena).  Tile t of list l goes from tile0_old[l] + t to tile0_new[l] + t: a list's occupied tiles keep
//     their order, and a partly filled last tile travels with its pad rows, which the appended rows then fill;
//   * the position of appended row i in its list: size_old[list] + its stable rank among the rows of the same list that came before it
//     in the call (grow_positions: a cursor per list, carried from chunk to chunk).
#pragma once

#include <stdint.h>
#include <algorithm>
#include <vector>

namespace knnx {

constexpr uint32_t GROW_NO_TILE = 0xffffffffu;
constexpr int64_t GROW_MAX_PROWS = (int64_t)0xffffffffll;  // padded rows of one arena (arena rows are 32-bit: idmap / inv / hit lists)

enum { GROW_OK = 0, GROW_E_NEGATIVE = 1, GROW_E_ROWS = 2, GROW_E_LIST = 3 };

struct GrowPlan {
  std::vector<unsigned> tile0, ntile, size;  // the new layout [nlist]
  std::vector<uint32_t> src_tile;            // [max(tiles, 1)]
  int64_t rows = 0, tiles = 0, prow = 0;     // rows the lists hold; tiles and rows of the new padded arena (prow >= 32)
  int64_t old_rows = 0, old_tiles = 0;       // the same of the old layout
  int64_t moved_tiles = 0;                   // new tiles that have a source
};

// the layout of knnx_ivf_begin for these sizes (tile0 / ntile / size, rows, tiles, prow); GROW_E_ROWS past 2^32 padded rows
inline int grow_layout(int64_t nlist, const int64_t* sizes, std::vector<unsigned>& tile0, std::vector<unsigned>& ntile, std::vector<unsigned>& size,
                       int64_t& rows, int64_t& tiles, int64_t& prow) {
  const size_t nl = (size_t)std::max<int64_t>(nlist, 0);
  tile0.assign(nl, 0u), ntile.assign(nl, 0u), size.assign(nl, 0u);
  rows = tiles = 0;
  for (size_t l = 0; l < nl; ++l) {
    if (sizes[l] < 0) return GROW_E_NEGATIVE;
    const int64_t nt = (sizes[l] + 31) / 32;
    if ((tiles + nt) * 32 > GROW_MAX_PROWS) return GROW_E_ROWS;  // (checked before anything is narrowed to 32 bits)
    size[l] = (unsigned)sizes[l];
    ntile[l] = (unsigned)nt;
    tile0[l] = (unsigned)tiles;
    rows += sizes[l];
    tiles += nt;
  }
  prow = std::max<int64_t>(tiles * 32, 32);
  return GROW_OK;
}

// the plan for lists of size_old[l] rows that gain extra[l] >= 0 rows each
inline int grow_plan(int64_t nlist, const unsigned* size_old, const int64_t* extra, GrowPlan& p) {
  p = GrowPlan();
  const size_t nl = (size_t)std::max<int64_t>(nlist, 0);
  std::vector<int64_t> sum(nl);
  for (size_t l = 0; l < nl; ++l) {
    if (extra[l] < 0) return GROW_E_NEGATIVE;
    if (extra[l] > GROW_MAX_PROWS) return GROW_E_ROWS;
    sum[l] = (int64_t)size_old[l] + extra[l];
  }
  const int r = grow_layout(nlist, sum.data(), p.tile0, p.ntile, p.size, p.rows, p.tiles, p.prow);
  if (r) return r;
  p.src_tile.assign((size_t)std::max<int64_t>(p.tiles, 1), GROW_NO_TILE);
  for (size_t l = 0; l < nl; ++l) {
    const int64_t nt_old = ((int64_t)size_old[l] + 31) / 32;
    for (int64_t t = 0; t < nt_old; ++t) p.src_tile[(size_t)p.tile0[l] + (size_t)t] = (uint32_t)(p.old_tiles + t);
    p.old_tiles += nt_old;
    p.old_rows += (int64_t)size_old[l];
    p.moved_tiles += nt_old;
  }
  return GROW_OK;
}

// positions of n appended rows: pos[i] = cursor[lists[i]]++ (cursor [nlist] starts as size_old and is carried over the chunks of a call).
// GROW_E_LIST on a list id outside [0, nlist): nothing is written then, neither to pos nor to the cursor.
inline int grow_positions(int64_t nlist, const int32_t* lists, int64_t n, std::vector<int64_t>& cursor, int32_t* pos) {
  for (int64_t i = 0; i < n; ++i)
    if (lists[i] < 0 || (int64_t)lists[i] >= nlist) return GROW_E_LIST;
  for (int64_t i = 0; i < n; ++i) pos[i] = (int32_t)cursor[(size_t)lists[i]]++;
  return GROW_OK;
}

// extra[l] += rows of list l among lists [n]; GROW_E_LIST (extra untouched) on a list id outside [0, nlist)
inline int grow_count(int64_t nlist, const int32_t* lists, int64_t n, std::vector<int64_t>& extra) {
  for (int64_t i = 0; i < n; ++i)
    if (lists[i] < 0 || (int64_t)lists[i] >= nlist) return GROW_E_LIST;
  for (int64_t i = 0; i < n; ++i) extra[(size_t)lists[i]]++;
  return GROW_OK;
}

}  // namespace knnx
