// filter_plan_check.cpp -- drives csrc/knnx_filter_plan.h (tile enumeration, scratch sizes and the hook / compress rounds of the device
// post filter) on the CPU.  Its own main, only that header: built with -fsanitize=address,undefined by tests/test_filter_cpu.py and run
// as a child process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I clip-retrieval_amd/csrc tools/filter_plan_check.cpp -o filter_plan_check
// Prints one line per case and "filter plan ok" at the end; a failed check prints FAILED and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include <numeric>
#include <random>

#include "knnx_filter_plan.h"

using namespace knnx;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                \
    }                                                            \
  } while (0)

// the enumeration is usable in constant expressions (the kernels call the same function)
static_assert(filter_tile(0).ti == 0 && filter_tile(0).tj == 0, "tile 0");
static_assert(filter_tile(1).ti == 0 && filter_tile(1).tj == 1, "tile 1");
static_assert(filter_tile(2).ti == 1 && filter_tile(2).tj == 1, "tile 2");
static_assert(filter_tile(filter_tile_index(77, 127)).ti == 77 && filter_tile(filter_tile_index(77, 127)).tj == 127, "round trip");
static_assert(filter_tiles_side(FILTER_MAX_K) == 128 && filter_tiles(128) == 8256, "the largest request");

// every tile (ti <= tj < nt) exactly once, none outside
static void check_tiles(int nt) {
  std::vector<int> seen((size_t)nt * nt, 0);
  const int T = filter_tiles(nt);
  for (int t = 0; t < T; ++t) {
    const FilterTileXY xy = filter_tile(t);
    CHECK(xy.ti >= 0 && xy.ti <= xy.tj && xy.tj < nt);
    if (xy.ti < 0 || xy.tj >= nt || xy.ti > xy.tj) continue;
    CHECK(filter_tile_index(xy.ti, xy.tj) == t);
    ++seen[(size_t)xy.ti * nt + xy.tj];
  }
  int bad = 0;
  for (int i = 0; i < nt; ++i)
    for (int j = 0; j < nt; ++j) bad += seen[(size_t)i * nt + j] != (i <= j ? 1 : 0);
  CHECK(bad == 0);
}

// union-find answer: the smallest member of every node's component
static std::vector<int32_t> by_union_find(int n, const std::vector<uint32_t>& links) {
  std::vector<int32_t> p((size_t)n);
  std::iota(p.begin(), p.end(), 0);
  auto find = [&](int a) {
    while (p[(size_t)a] != a) a = p[(size_t)a] = p[(size_t)p[(size_t)a]];
    return a;
  };
  for (uint32_t l : links) {
    const int a = find(filter_link_i(l)), b = find(filter_link_j(l));
    if (a != b) p[(size_t)std::max(a, b)] = std::min(a, b);
  }
  std::vector<int32_t> out((size_t)n);
  for (int x = 0; x < n; ++x) out[(size_t)x] = find(x);
  return out;
}

static int worst_rounds = 0;
static void check_graph(const char* name, int n, std::vector<uint32_t> links, std::mt19937& rng, int shuffles = 4) {
  const std::vector<int32_t> want = by_union_find(n, links);
  int lo = 1 << 30, hi = 0;
  for (int s = 0; s <= shuffles; ++s) {
    if (s) std::shuffle(links.begin(), links.end(), rng);
    std::vector<int32_t> label;
    int rounds = -1;
    const int rc = filter_cc(n, links.data(), (int64_t)links.size(), label, rounds);
    CHECK(rc == 0);
    CHECK(rounds >= (n > 0 ? 1 : 0) && rounds <= std::max(n, 0));
    CHECK(label == want);
    lo = std::min(lo, rounds), hi = std::max(hi, rounds);
  }
  worst_rounds = std::max(worst_rounds, hi);
  if (name) printf("graph %-34s n %5d links %7zu rounds %d..%d\n", name, n, links.size(), lo, hi);
}

static uint32_t L(int a, int b) { return filter_link(std::min(a, b), std::max(a, b)); }

int main() {
  for (int nt = 1; nt <= 130; ++nt) check_tiles(nt);
  printf("tiles: every tile of the triangle once for nt = 1 .. 130\n");
  for (int n : {1, 63, 64, 65, 128, 129, 3000, 8191, 8192}) CHECK(filter_tiles_side(n) == (n + 63) / 64);

  const FilterSizes z = filter_sizes(3000, 1024, 2, 1);
  CHECK(z.rows == (size_t)3000 * 1024 && z.ids == 3000 && z.links == ((size_t)1 << 20) && z.vscores == 6000 && z.sscores == 3000 && z.drop == 3000);
  CHECK(z.bytes() == (size_t)3000 * 1024 * 4 + 3000 * 8 + ((size_t)4 << 20) + FILTER_COUNTERS * 4 + 6000 * 4 + 3000 * 4 + 3000);
  CHECK(filter_sizes(8192, 4096, 0, 0).vscores == 8192);  // (no model: one float per row, never an empty allocation)
  printf("sizes: k 3000 d 1024 -> %zu bytes\n", z.bytes());

  std::mt19937 rng(12345);
  check_graph("empty", 0, {}, rng);
  check_graph("one node", 1, {}, rng);
  check_graph("no links", 500, {}, rng);
  for (int n : {2, 3, 64, 150, 1000, 8192}) {
    std::vector<uint32_t> path, rpath, star, hub_last;
    for (int i = 0; i + 1 < n; ++i) path.push_back(L(i, i + 1));
    for (int i = 1; i < n; ++i) star.push_back(L(0, i)), hub_last.push_back(L(i - 1, n - 1));
    check_graph("path", n, path, rng);
    check_graph("star around the smallest", n, star, rng);
    check_graph("star around the largest", n, hub_last, rng);
    // a path whose ranks are scrambled along it: the smallest label has to travel both ways
    std::vector<int> perm((size_t)n);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), rng);
    for (int i = 0; i + 1 < n; ++i) rpath.push_back(L(perm[(size_t)i], perm[(size_t)i + 1]));
    check_graph("path in scrambled ranks", n, rpath, rng);
  }
  for (int n : {2, 5, 40, 300}) {
    std::vector<uint32_t> clique;
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) clique.push_back(L(i, j));
    check_graph("clique", n, clique, rng);
  }
  {  // two components (evens, odds: each a path) joined by ONE link between their largest members
    const int n = 2000;
    std::vector<uint32_t> two;
    for (int i = 0; i + 2 < n; ++i) two.push_back(L(i, i + 2));
    check_graph("two paths, not joined", n, two, rng);
    two.push_back(L(n - 2, n - 1));
    check_graph("two paths joined at their largest", n, two, rng);
  }
  for (int rep = 0; rep < 300; ++rep) {
    const int n = 2 + (int)(rng() % 400);
    const int m = (int)(rng() % (unsigned)(2 * n));
    std::vector<uint32_t> links;
    for (int e = 0; e < m; ++e) {
      const int a = (int)(rng() % (unsigned)n), b = (int)(rng() % (unsigned)n);
      if (a != b) links.push_back(L(a, b));
    }
    check_graph(rep < 3 ? "random" : nullptr, n, links, rng, 2);
  }
  printf("random graphs: 300, worst rounds over everything %d\n", worst_rounds);
  if (failures) {
    printf("%d checks FAILED\n", failures);
    return 1;
  }
  printf("filter plan ok\n");
  return 0;
}
