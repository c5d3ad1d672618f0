// shrink_plan_check.cpp -- drives csrc/knnx_shrink_plan.h (the integer arithmetic of removing ids from a built IVF index: the block-sum
// scan, the mask -> position rule, dst0, the consistency checks) on the CPU, step by step as the device runs it, against the plain
// sequential shrink_reference of the same header.  Its own main, only that header: built with -fsanitize=address,undefined by
// tests/test_ivf_remove_cpu.py and run as a child process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I clip-retrieval_amd/csrc tools/shrink_plan_check.cpp -o shrink_plan_check
// Prints one line per case and "shrink plan ok" at the end; a failed check prints FAILED and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include <numeric>
#include <string>

#include "knnx_shrink_plan.h"

using namespace knnx;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                \
    }                                                            \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return rng_state * 0x2545f4914f6cdd1dull;
}

// an index of these list sizes whose ids are dealt to the lists in a shuffled order, ascending inside a list (the position rule of the
// build): idmap [prow], -1 on pad rows
struct Index {
  std::vector<unsigned> size, tile0, ntile;
  std::vector<int64_t> idmap;
  int64_t n = 0, prow = 0, id_lo = 0;
};
static Index make_index(const std::vector<unsigned>& size, int64_t id_lo) {
  Index ix;
  ix.size = size, ix.id_lo = id_lo;
  std::vector<int64_t> s64(size.begin(), size.end());
  int64_t tiles = 0;
  std::vector<unsigned> sz;
  CHECK(grow_layout((int64_t)size.size(), s64.data(), ix.tile0, ix.ntile, sz, ix.n, tiles, ix.prow) == GROW_OK);
  std::vector<int32_t> list_of((size_t)ix.n);
  size_t k = 0;
  for (size_t l = 0; l < size.size(); ++l)
    for (unsigned j = 0; j < size[l]; ++j) list_of[k++] = (int32_t)l;
  for (size_t i = list_of.size(); i > 1; --i) std::swap(list_of[i - 1], list_of[(size_t)(rnd() % i)]);
  ix.idmap.assign((size_t)ix.prow, -1);
  std::vector<int64_t> fill(size.size(), 0);
  for (int64_t i = 0; i < ix.n; ++i) {
    const size_t l = (size_t)list_of[(size_t)i];
    ix.idmap[(size_t)(32 * (int64_t)ix.tile0[l] + fill[l]++)] = id_lo + i;
  }
  return ix;
}

// the device sequence on the host, piece by piece, against shrink_reference
static void check_case(const std::string& name, const Index& ix, const std::vector<uint8_t>& dead) {
  const int64_t nlist = (int64_t)ix.size.size(), n = ix.n;
  ShrinkRef R;
  CHECK(shrink_reference(nlist, ix.size.data(), ix.idmap.data(), ix.id_lo, n, dead.data(), R) == SHRINK_OK);
  // rank: block sums, their scan, the ranks
  std::vector<uint32_t> sums, off, rank;
  shrink_block_sums(dead.data(), n, sums);
  int64_t survivors = -1;
  CHECK(shrink_block_scan(sums.data(), (int64_t)sums.size(), n, off, survivors) == SHRINK_OK);
  CHECK(survivors == R.rows);
  shrink_ranks(dead.data(), n, off, rank);
  // masks, positions, sizes
  std::vector<uint32_t> tmask, tpos;
  std::vector<int64_t> size_new;
  shrink_masks(ix.idmap.data(), ix.prow, ix.id_lo, n, dead.data(), tmask);
  shrink_list_scan(nlist, ix.tile0.data(), ix.ntile.data(), tmask, tpos, size_new);
  std::vector<unsigned> tile0, ntile, size;
  int64_t tiles = 0, prow = 0;
  CHECK(shrink_layout(nlist, ix.size.data(), size_new.data(), survivors, ix.prow, tile0, ntile, size, tiles, prow) == SHRINK_OK);
  CHECK(tile0 == R.tile0 && ntile == R.ntile && size == R.size && tiles == R.tiles && prow == R.prow);
  CHECK(shrink_layout(nlist, ix.size.data(), size_new.data(), survivors + 1, ix.prow, tile0, ntile, size, tiles, prow) == SHRINK_E_COUNT);
  shrink_dst0(nlist, ix.tile0.data(), ix.ntile.data(), tile0.data(), tpos);
  // every source row: where it goes and the id it gets; every destination row is written once
  std::vector<int64_t> idmap((size_t)prow, -1);
  std::vector<uint32_t> inv((size_t)survivors, 0xffffffffu);
  int64_t moved = 0;
  bool runs_ok = true;
  for (int64_t r = 0; r < ix.prow; ++r) {
    const uint32_t m = tmask[(size_t)(r >> 5)];
    const unsigned b = (unsigned)(r & 31);
    if (!((m >> b) & 1u)) {
      runs_ok = runs_ok && R.dest[(size_t)r] == -1;
      continue;
    }
    const int64_t dest = (int64_t)tpos[(size_t)(r >> 5)] + shrink_pos(m, b);
    const uint64_t o = shrink_index(ix.idmap[(size_t)r], ix.id_lo, n);
    runs_ok = runs_ok && dest == R.dest[(size_t)r] && dest < prow && o < (uint64_t)n && idmap[(size_t)dest] == -1;
    if (dest >= prow || o >= (uint64_t)n) continue;
    idmap[(size_t)dest] = ix.id_lo + rank[o];
    if (rank[o] < inv.size()) inv[rank[o]] = (uint32_t)dest;
    ++moved;
  }
  CHECK(runs_ok);
  CHECK(moved == survivors);
  CHECK(idmap == R.idmap);
  CHECK(inv == R.inv);
  // the survivors of a list are in ascending id order and the pad rows are the tail of its last tile
  bool order_ok = true;
  for (int64_t l = 0; l < nlist; ++l)
    for (int64_t j = 0; j < 32 * (int64_t)ntile[(size_t)l]; ++j) {
      const int64_t id = idmap[(size_t)(32 * (int64_t)tile0[(size_t)l] + j)];
      order_ok = order_ok && (j < (int64_t)size[(size_t)l] ? id >= ix.id_lo && (j == 0 || id > idmap[(size_t)(32 * (int64_t)tile0[(size_t)l] + j - 1)]) : id == -1);
    }
  CHECK(order_ok);
  printf("%s: lists %lld rows %lld -> %lld tiles %lld -> %lld\n", name.c_str(), (long long)nlist, (long long)n, (long long)survivors,
         (long long)(ix.prow / 32), (long long)tiles);
}

static std::vector<uint8_t> dead_of(const Index& ix, const std::vector<std::pair<int, int>>& list_pos) {  // (list, position)
  std::vector<uint8_t> dead((size_t)ix.n, 0);
  for (const auto& lp : list_pos) dead[(size_t)(ix.idmap[(size_t)(32 * (int64_t)ix.tile0[(size_t)lp.first] + lp.second)] - ix.id_lo)] = 1;
  return dead;
}

int main() {
  const std::vector<unsigned> crafted = {0, 1, 31, 32, 33, 700, 64, 65, 96, 0, 5, 130, 17, 250, 2, 63, 40, 128, 90, 11, 160, 75, 1, 300};
  for (int64_t id_lo : {(int64_t)0, (int64_t)1000}) {
    const Index ix = make_index(crafted, id_lo);
    std::vector<std::pair<int, int>> s = {{1, 0}, {2, 0}, {3, 31}, {4, 0}, {5, 0}, {5, 699}, {23, 299}};
    for (int j = 32; j < 64; ++j) s.push_back({5, j});
    for (int j = 100; j <= 400; j += 3) s.push_back({5, j});
    for (int j = 0; j < 64; j += 2) s.push_back({6, j});
    for (int j = 0; j < 65; ++j) s.push_back({7, j});
    for (int j = 0; j < 32; ++j) s.push_back({8, j});
    for (int j = 0; j < 249; ++j) s.push_back({13, j});
    check_case("crafted removal, id_base " + std::to_string(id_lo), ix, dead_of(ix, s));
    check_case("crafted nothing dead, id_base " + std::to_string(id_lo), ix, std::vector<uint8_t>((size_t)ix.n, 0));
    check_case("crafted everything dead, id_base " + std::to_string(id_lo), ix, std::vector<uint8_t>((size_t)ix.n, 1));
    std::vector<uint8_t> one((size_t)ix.n, 0);
    one[0] = 1;
    check_case("crafted first id dead, id_base " + std::to_string(id_lo), ix, one);
  }
  {
    const Index empty = make_index(std::vector<unsigned>(5, 0u), 7);
    check_case("empty index of empty lists", empty, std::vector<uint8_t>());
  }
  // ids that name no row
  CHECK(shrink_index(-1, 0, 10) == 10 && shrink_index(10, 0, 10) == 10 && shrink_index(9, 0, 10) == 9 && shrink_index(999, 1000, 10) == 10);
  CHECK(shrink_index(INT64_MIN, 1000, 10) == 10 && shrink_index(INT64_MAX, 1000, 10) == 10 && shrink_index(1009, 1000, 10) == 9);
  printf("ids that name no row\n");
  // the mask -> position rule, every bit of a few masks
  for (uint32_t m : {0u, 1u, 0x80000000u, 0xffffffffu, 0x55555555u, 0xf0f0a5c3u}) {
    unsigned run = 0;
    for (unsigned b = 0; b < 32; ++b) {
      CHECK(shrink_pos(m, b) == run);
      run += (m >> b) & 1u;
    }
  }
  printf("mask positions\n");
  // refusals of the checks: a block with too many survivors, sizes that do not add up, a list that grows
  {
    std::vector<uint32_t> off;
    int64_t total = 0;
    const uint32_t bad[2] = {1024, 1025};
    CHECK(shrink_block_scan(bad, 2, 4096, off, total) == SHRINK_E_COUNT);
    const uint32_t many[2] = {1024, 1024};
    CHECK(shrink_block_scan(many, 2, 2047, off, total) == SHRINK_E_COUNT);
    CHECK(shrink_block_scan(many, 2, 2048, off, total) == SHRINK_OK && total == 2048 && off[1] == 1024);
    const unsigned so[2] = {10, 40};
    const int64_t grows[2] = {11, 0}, fine[2] = {10, 3};
    std::vector<unsigned> a, b, c;
    int64_t tiles = 0, prow = 0;
    CHECK(shrink_layout(2, so, grows, 11, 96, a, b, c, tiles, prow) == SHRINK_E_LAYOUT);
    CHECK(shrink_layout(2, so, fine, 12, 96, a, b, c, tiles, prow) == SHRINK_E_COUNT);
    CHECK(shrink_layout(2, so, fine, 13, 96, a, b, c, tiles, prow) == SHRINK_OK && prow == 64 && a[1] == 1);
    printf("refusal inconsistent counts\n");
  }
  // random layouts: all rows dead, no rows dead, whole tiles dead, empty lists at both ends, a list far longer than the others
  int cases = 0;
  for (int it = 0; it < 3000; ++it) {
    const int nlist = 1 + (int)(rnd() % 12);
    std::vector<unsigned> size((size_t)nlist);
    for (unsigned& s : size) {
      const unsigned kind = (unsigned)(rnd() % 6);
      s = kind == 0 ? 0u : kind == 1 ? 32u * (unsigned)(rnd() % 4) : kind == 2 ? (unsigned)(rnd() % 2500) : (unsigned)(rnd() % 100);
    }
    if (it % 4 == 1) size.front() = 0, size.back() = 0;
    const Index ix = make_index(size, (int64_t)(rnd() % 3) * 500);
    std::vector<uint8_t> dead((size_t)ix.n, 0);
    const int mode = it % 6;
    if (mode == 0) dead.assign((size_t)ix.n, 1);
    else if (mode == 2 || mode == 3) {
      const unsigned p = 1 + (unsigned)(rnd() % 99);
      for (uint8_t& x : dead) x = rnd() % 100 < p;
    }
    if (mode == 3 || mode == 4)  // whole tiles
      for (int64_t t = 0; t < ix.prow / 32; ++t)
        if (rnd() % 3 == 0)
          for (int b = 0; b < 32; ++b)
            if (ix.idmap[(size_t)(32 * t + b)] >= 0) dead[(size_t)(ix.idmap[(size_t)(32 * t + b)] - ix.id_lo)] = 1;
    const int before = failures;
    if (it < 12) check_case("random " + std::to_string(it), ix, dead);
    else {  // (quiet: one line for all of them below)
      ShrinkRef R;
      std::vector<uint32_t> sums, off, rank, tmask, tpos;
      std::vector<int64_t> size_new;
      std::vector<unsigned> tile0, ntile, sz;
      int64_t survivors = 0, tiles = 0, prow = 0;
      CHECK(shrink_reference(nlist, ix.size.data(), ix.idmap.data(), ix.id_lo, ix.n, dead.data(), R) == SHRINK_OK);
      shrink_block_sums(dead.data(), ix.n, sums);
      CHECK(shrink_block_scan(sums.data(), (int64_t)sums.size(), ix.n, off, survivors) == SHRINK_OK && survivors == R.rows);
      shrink_ranks(dead.data(), ix.n, off, rank);
      shrink_masks(ix.idmap.data(), ix.prow, ix.id_lo, ix.n, dead.data(), tmask);
      shrink_list_scan(nlist, ix.tile0.data(), ix.ntile.data(), tmask, tpos, size_new);
      CHECK(shrink_layout(nlist, ix.size.data(), size_new.data(), survivors, ix.prow, tile0, ntile, sz, tiles, prow) == SHRINK_OK);
      CHECK(tile0 == R.tile0 && sz == R.size && prow == R.prow);
      shrink_dst0(nlist, ix.tile0.data(), ix.ntile.data(), tile0.data(), tpos);
      std::vector<int64_t> idmap((size_t)prow, -1);
      std::vector<uint32_t> inv((size_t)survivors, 0xffffffffu);
      bool ok = true;
      for (int64_t r = 0; r < ix.prow && ok; ++r) {
        const uint32_t m = tmask[(size_t)(r >> 5)];
        if (!((m >> (r & 31)) & 1u)) continue;
        const int64_t dest = (int64_t)tpos[(size_t)(r >> 5)] + shrink_pos(m, (unsigned)(r & 31));
        const uint64_t o = shrink_index(ix.idmap[(size_t)r], ix.id_lo, ix.n);
        ok = dest < prow && o < (uint64_t)ix.n && rank[o] < inv.size() && idmap[(size_t)dest] == -1;
        if (ok) idmap[(size_t)dest] = ix.id_lo + rank[o], inv[rank[o]] = (uint32_t)dest;
      }
      CHECK(ok && idmap == R.idmap && inv == R.inv);
    }
    cases += failures == before;
  }
  printf("random layouts: %d of 3000 agree with the reference\n", cases);
  CHECK(cases == 3000);
  if (failures) {
    printf("%d checks FAILED\n", failures);
    return 1;
  }
  printf("shrink plan ok\n");
  return 0;
}
