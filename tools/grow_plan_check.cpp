// grow_plan_check.cpp -- drives csrc/knnx_grow_plan.h (the host plan of growing a built IVF index: the new layout, the tile source table,
// the positions of appended rows, the 2^32 padded-row limit) on the CPU.  Its own main, only that header: built with
// -fsanitize=address,undefined by tests/test_ivf_append_cpu.py and run as a child process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I clip-retrieval_amd/csrc tools/grow_plan_check.cpp -o grow_plan_check
// Prints one line per case and "grow plan ok" at the end; a failed check prints FAILED and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include "knnx_grow_plan.h"

using namespace knnx;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                \
    }                                                            \
  } while (0)

// the layout rule of knnx_ivf_begin (knnx_ivf.hip: ivf_tile_layout), restated with a plain loop
struct Ref {
  std::vector<unsigned> tile0, ntile, size;
  int64_t rows = 0, tiles = 0, prow = 0;
};
static Ref ref_layout(const std::vector<int64_t>& sizes) {
  Ref t;
  for (size_t l = 0; l < sizes.size(); ++l) {
    t.size.push_back((unsigned)sizes[l]);
    t.ntile.push_back((unsigned)((sizes[l] + 31) / 32));
    t.tile0.push_back((unsigned)t.tiles);
    t.rows += sizes[l];
    t.tiles += (sizes[l] + 31) / 32;
  }
  t.prow = t.tiles * 32 > 32 ? t.tiles * 32 : 32;
  return t;
}

static void check_plan(const char* name, const std::vector<unsigned>& size_old, const std::vector<int64_t>& extra) {
  const int64_t nlist = (int64_t)size_old.size();
  GrowPlan p;
  CHECK(grow_plan(nlist, size_old.data(), extra.data(), p) == GROW_OK);
  std::vector<int64_t> so(size_old.begin(), size_old.end()), sum(size_old.size());
  for (size_t l = 0; l < sum.size(); ++l) sum[l] = so[l] + extra[l];
  const Ref o = ref_layout(so), n = ref_layout(sum);
  // the new layout is the build's layout of the summed sizes
  CHECK(p.tile0 == n.tile0 && p.ntile == n.ntile && p.size == n.size);
  CHECK(p.rows == n.rows && p.tiles == n.tiles && p.prow == n.prow);
  CHECK(p.old_rows == o.rows && p.old_tiles == o.tiles && p.moved_tiles == o.tiles);
  CHECK((int64_t)p.src_tile.size() == (n.tiles > 1 ? n.tiles : 1));
  // every old tile is the source of exactly one new tile, the t-th tile of the same list; every other new tile has none
  std::vector<int> seen((size_t)o.tiles, 0);
  int64_t none = 0;
  for (size_t t = 0; t < p.src_tile.size(); ++t) {
    const uint32_t s = p.src_tile[t];
    if (s == GROW_NO_TILE) {
      ++none;
      continue;
    }
    CHECK((int64_t)s < o.tiles);
    if ((int64_t)s < o.tiles) seen[s]++;
  }
  for (size_t s = 0; s < seen.size(); ++s) CHECK(seen[s] == 1);
  CHECK(none == (int64_t)p.src_tile.size() - o.tiles);
  for (int64_t l = 0; l < nlist; ++l)
    for (unsigned t = 0; t < n.ntile[(size_t)l]; ++t) {
      const uint32_t s = p.src_tile[(size_t)n.tile0[(size_t)l] + t];
      if (t < o.ntile[(size_t)l]) CHECK(s == o.tile0[(size_t)l] + t);
      else CHECK(s == GROW_NO_TILE);
    }
  printf("plan %-32s nlist %3lld rows %7lld -> %7lld tiles %5lld -> %5lld moved %5lld\n", name, (long long)nlist, (long long)o.rows,
         (long long)n.rows, (long long)o.tiles, (long long)n.tiles, (long long)p.moved_tiles);
}

// positions against the definition: size_old[list] + the number of earlier rows of the call in the same list, over ragged chunks
static void check_positions(const char* name, const std::vector<unsigned>& size_old, const std::vector<int32_t>& lists, int64_t chunk) {
  const int64_t nlist = (int64_t)size_old.size(), n = (int64_t)lists.size();
  std::vector<int64_t> cursor(size_old.begin(), size_old.end()), extra((size_t)nlist, 0);
  std::vector<int32_t> pos((size_t)n, -7);
  for (int64_t o = 0; o < n; o += chunk) {
    const int64_t m = n - o < chunk ? n - o : chunk;
    CHECK(grow_positions(nlist, lists.data() + o, m, cursor, pos.data() + o) == GROW_OK);
  }
  CHECK(grow_count(nlist, lists.data(), n, extra) == GROW_OK);
  for (int64_t i = 0; i < n; ++i) {
    int64_t rank = 0;
    for (int64_t j = 0; j < i; ++j) rank += lists[(size_t)j] == lists[(size_t)i];
    CHECK(pos[(size_t)i] == (int64_t)size_old[(size_t)lists[(size_t)i]] + rank);
  }
  for (int64_t l = 0; l < nlist; ++l) CHECK(cursor[(size_t)l] == (int64_t)size_old[(size_t)l] + extra[(size_t)l]);
  printf("positions %-27s rows %5lld chunk %5lld\n", name, (long long)n, (long long)chunk);
}

int main() {
  // the crafted lists of the GPU test: every tile boundary a list can cross or reach
  const std::vector<unsigned> crafted = {0, 1, 31, 32, 33, 700, 5, 64, 0, 100};
  check_plan("crafted growth", crafted, {1, 31, 1, 1, 31, 300, 0, 0, 0, 7});
  check_plan("extra counts all zero", crafted, std::vector<int64_t>(crafted.size(), 0));
  check_plan("empty index of empty lists", std::vector<unsigned>(7, 0u), {0, 3, 0, 0, 40, 0, 1});
  check_plan("empty index, nothing added", std::vector<unsigned>(5, 0u), std::vector<int64_t>(5, 0));
  check_plan("one list takes everything", crafted, {0, 0, 0, 0, 0, 0, 100000, 0, 0, 0});
  check_plan("first and last list grow", crafted, {33, 0, 0, 0, 0, 0, 0, 0, 0, 29});
  check_plan("a single list", {95}, {2});
  {
    unsigned x = 12345u;  // a fixed pseudo-random case
    std::vector<unsigned> so(97);
    std::vector<int64_t> ex(97);
    for (size_t l = 0; l < so.size(); ++l) {
      x = x * 1664525u + 1013904223u;
      so[l] = (x >> 8) % 5 == 0 ? 0u : (x >> 8) % 300;
      x = x * 1664525u + 1013904223u;
      ex[l] = (x >> 8) % 3 == 0 ? 0 : (int64_t)((x >> 8) % 90);
    }
    check_plan("pseudo-random, 97 lists", so, ex);
  }
  // positions
  {
    std::vector<int32_t> lists;
    unsigned x = 99u;
    for (int i = 0; i < 500; ++i) {
      x = x * 1664525u + 1013904223u;
      lists.push_back((int32_t)((x >> 10) % crafted.size()));
    }
    check_positions("random lists, one chunk", crafted, lists, 1000);
    check_positions("random lists, chunks of 64", crafted, lists, 64);
    check_positions("random lists, chunks of 1", crafted, lists, 1);
    check_positions("one list takes everything", crafted, std::vector<int32_t>(300, 6), 128);
    check_positions("no rows", crafted, std::vector<int32_t>(), 16);
  }
  // refusals: nothing is written
  {
    std::vector<int64_t> cursor(crafted.begin(), crafted.end()), extra(crafted.size(), 0);
    const std::vector<int64_t> cursor0 = cursor;
    std::vector<int32_t> pos(3, -7);
    const int32_t bad_hi[3] = {1, (int32_t)crafted.size(), 2}, bad_lo[3] = {1, 2, -1};
    CHECK(grow_positions((int64_t)crafted.size(), bad_hi, 3, cursor, pos.data()) == GROW_E_LIST);
    CHECK(grow_positions((int64_t)crafted.size(), bad_lo, 3, cursor, pos.data()) == GROW_E_LIST);
    CHECK(grow_count((int64_t)crafted.size(), bad_hi, 3, extra) == GROW_E_LIST);
    CHECK(grow_count((int64_t)crafted.size(), bad_lo, 3, extra) == GROW_E_LIST);
    CHECK(cursor == cursor0 && pos == std::vector<int32_t>(3, -7) && extra == std::vector<int64_t>(crafted.size(), 0));
    printf("refusal list id out of range\n");
    GrowPlan p;
    CHECK(grow_plan(2, crafted.data(), std::vector<int64_t>{0, -1}.data(), p) == GROW_E_NEGATIVE);
    printf("refusal negative extra count\n");
  }
  // the 2^32 padded-row limit: 2^27 - 1 full tiles are the most an arena holds (prow = 2^32 - 32)
  {
    const int64_t most = (((int64_t)1 << 27) - 1) * 32;
    GrowPlan p;
    const unsigned one[1] = {0u};
    const int64_t fits[1] = {most}, over[1] = {most + 1};
    // (only the layout half is driven at this size: the source table of 2^27 tiles is 512 MiB)
    std::vector<unsigned> t0, nt, sz;
    int64_t rows, tiles, prow;
    CHECK(grow_layout(1, fits, t0, nt, sz, rows, tiles, prow) == GROW_OK && prow == most && tiles == ((int64_t)1 << 27) - 1);
    CHECK(grow_layout(1, over, t0, nt, sz, rows, tiles, prow) == GROW_E_ROWS);
    CHECK(grow_plan(1, one, over, p) == GROW_E_ROWS);
    // the PAD rows count: 2^32 - 16 rows in one list are 2^27 tiles, one too many, whatever is appended elsewhere
    const unsigned two[2] = {0xfffffff0u, 0u};
    const int64_t pad_over[2] = {0, 17};
    CHECK(grow_plan(2, two, pad_over, p) == GROW_E_ROWS);
    const int64_t huge[1] = {(int64_t)1 << 40};
    CHECK(grow_plan(1, one, huge, p) == GROW_E_ROWS);
    printf("refusal 2^32 padded rows\n");
  }
  if (failures) {
    printf("%d checks FAILED\n", failures);
    return 1;
  }
  printf("grow plan ok\n");
  return 0;
}
