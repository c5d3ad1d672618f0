// knnx_id_order.h -- the host arithmetic of the list-ordered ids of an IVF index (knnx_ivf_id_order / knnx_ivf_map_ids and their
// knnx_shards_* forms; include/knnx.h, "List-ordered ids").  No device code in here: plain 64-bit arithmetic on list sizes, ids and row
// ranges, so that a host-only program can drive it (tools/id_order_check.cpp).
//
// List l of a built index holds size[l] rows at arena rows 32 * tile0[l] + j, j < size[l].  dense0[l] = the exclusive prefix sum of size
// (int64, nlist + 1 entries, the last one = ntotal); the ORDINAL of the row at position j of list l is dense0[l] + j.  Pad rows have none.
// An arena row p belongs to the LAST list with tile0[l] <= p / 32: empty lists share their tile0 with the list after them and trailing
// empty lists carry the tile count, so "the last one" is the list that owns the tile.  The same holds for an ordinal o and dense0.
#pragma once

#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

// (the kernel file defines this as a host + device function before it includes the header: one search serves both sides)
#ifndef KNNX_IDO_FN
#define KNNX_IDO_FN inline
#endif

namespace knnx {

// the largest l in [0, n) with a[l] <= v; a ascending, a[0] <= v required (a[0] = 0 for tile0 and dense0)
template <class T>
KNNX_IDO_FN int ido_last_le(const T* a, int n, T v) {
  int lo = 0, hi = n;  // a[lo] <= v < a[hi] (a[n] = +inf)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the ordinal of arena row p (a row of a list, not a pad row)
KNNX_IDO_FN int64_t ido_ordinal_of_row(const unsigned* tile0, const int64_t* dense0, int nlist, uint32_t p) {
  const int l = ido_last_le<unsigned>(tile0, nlist, p >> 5);
  return dense0[l] + ((int64_t)p - (int64_t)tile0[l] * 32);
}

// the arena row of ordinal o in [0, ntotal)
KNNX_IDO_FN int64_t ido_row_of_ordinal(const unsigned* tile0, const int64_t* dense0, int nlist, int64_t o) {
  const int l = ido_last_le<int64_t>(dense0, nlist, o);
  return (int64_t)tile0[l] * 32 + (o - dense0[l]);
}

// dense0 [nlist + 1] from the list sizes
inline void ido_dense0(const unsigned* size, int64_t nlist, std::vector<int64_t>& dense0) {
  dense0.assign((size_t)std::max<int64_t>(nlist, 0) + 1, 0);
  for (int64_t l = 0; l < nlist; ++l) dense0[(size_t)l + 1] = dense0[(size_t)l] + (int64_t)size[l];
}

// ---- the chunk plan of the export: consecutive ranges of `chunk` ordinals (ids for old_to_new), the last one ragged ----------------
constexpr int64_t IDO_CHUNK_DEFAULT = (int64_t)1 << 22;  // 32 MiB of int64 in the staging buffer
constexpr int64_t IDO_CHUNK_MIN = 64;
// KNNX_ID_ORDER_CHUNK as the environment gives it (null / empty / not a number: the default; below the minimum: the minimum)
inline int64_t ido_chunk_from_env(const char* v) {
  if (!v || !v[0]) return IDO_CHUNK_DEFAULT;
  char* end = nullptr;
  const long long c = strtoll(v, &end, 10);
  if (end == v) return IDO_CHUNK_DEFAULT;
  return std::max<int64_t>((int64_t)c, IDO_CHUNK_MIN);
}
struct IdoChunks {
  int64_t total = 0, chunk = IDO_CHUNK_DEFAULT;
  IdoChunks() {}
  IdoChunks(int64_t total_, int64_t chunk_) : total(std::max<int64_t>(total_, 0)), chunk(std::max<int64_t>(chunk_, 1)) {}
  int64_t count() const { return (total + chunk - 1) / chunk; }
  int64_t first(int64_t i) const { return i * chunk; }
  int64_t len(int64_t i) const { return std::min(chunk, total - i * chunk); }
  int64_t staging() const { return std::min(chunk, total); }  // entries the staging buffer holds
};

// ---- the range check of knnx_ivf_map_ids: the position of the first id that is neither -1 nor in [id_base, id_base + ntotal); -1: none
inline int64_t ido_first_bad(const int64_t* ids, int64_t n, int64_t id_base, int64_t ntotal) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t v = ids[i];
    if (v == -1) continue;
    // (v - id_base could wrap for ids near the ends of int64: compare without subtracting)
    if (v < id_base || v >= id_base + ntotal) return i;
  }
  return -1;
}

// ---- shard routing of knnx_shards_map_ids: shard g owns the ids [lo[g], hi[g]) ----------------------------------------------------
struct IdoRoute {
  std::vector<std::vector<int64_t>> ids;  // per shard: the ids routed to it, in request order
  std::vector<std::vector<int64_t>> pos;  // ... and where each of them stood in the request
};
// partition by row range; -1 goes to no shard (it maps to -1).  Returns the position of the first id no shard owns, or -1.
inline int64_t ido_route(const int64_t* ids, int64_t n, const int64_t* lo, const int64_t* hi, int P, IdoRoute& r) {
  r.ids.assign((size_t)std::max(P, 0), std::vector<int64_t>());
  r.pos.assign((size_t)std::max(P, 0), std::vector<int64_t>());
  for (int64_t i = 0; i < n; ++i) {
    const int64_t v = ids[i];
    if (v == -1) continue;
    int g = 0;
    while (g < P && !(v >= lo[g] && v < hi[g])) ++g;
    if (g == P) return i;
    r.ids[(size_t)g].push_back(v);
    r.pos[(size_t)g].push_back(i);
  }
  return -1;
}
// put shard g's answers (mapped[j] for r.ids[g][j]) back in request order
inline void ido_scatter_back(const IdoRoute& r, int g, const int64_t* mapped, int64_t* out) {
  const std::vector<int64_t>& p = r.pos[(size_t)g];
  for (size_t j = 0; j < p.size(); ++j) out[p[j]] = mapped[j];
}

}  // namespace knnx
