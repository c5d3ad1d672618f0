// id_order_check.cpp -- drives csrc/knnx_id_order.h (the host arithmetic of the list-ordered ids: dense0, the list searches, the chunk
// plan of the export, the range check, the shard routing) on the CPU.  Its own main, only that header: built with
// -fsanitize=address,undefined by tests/test_ivf_id_order_cpu.py and run as a child process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I clip-retrieval_amd/csrc tools/id_order_check.cpp -o id_order_check
// Prints one line per case and "id order ok" at the end; a failed check prints FAILED and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include "knnx_id_order.h"

using namespace knnx;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                \
    }                                                            \
  } while (0)

// dense0 against a plain loop, and both searches against a walk over every row of every list: the arena row of ordinal o and the
// ordinal of that row, with empty lists wherever the case puts them
static void check_dense0(const char* name, const std::vector<unsigned>& size) {
  const int nlist = (int)size.size();
  std::vector<int64_t> d0;
  ido_dense0(size.data(), nlist, d0);
  std::vector<unsigned> tile0((size_t)nlist);
  unsigned tiles = 0;
  for (int l = 0; l < nlist; ++l) tile0[(size_t)l] = tiles, tiles += (size[(size_t)l] + 31) / 32;
  CHECK((int)d0.size() == nlist + 1 && d0[0] == 0);
  int64_t o = 0;
  for (int l = 0; l < nlist; ++l) {
    CHECK(d0[(size_t)l] == o);
    for (unsigned j = 0; j < size[(size_t)l]; ++j, ++o) {
      const int64_t row = (int64_t)tile0[(size_t)l] * 32 + j;
      CHECK(ido_row_of_ordinal(tile0.data(), d0.data(), nlist, o) == row);
      CHECK(ido_ordinal_of_row(tile0.data(), d0.data(), nlist, (uint32_t)row) == o);
      CHECK(ido_last_le<unsigned>(tile0.data(), nlist, (unsigned)(row >> 5)) == l);
      CHECK(ido_last_le<int64_t>(d0.data(), nlist, o) == l);
    }
  }
  CHECK(d0[(size_t)nlist] == o);
  printf("dense0 %-34s nlist %3d rows %6lld tiles %4u\n", name, nlist, (long long)o, tiles);
}

// every ordinal of [0, total) is covered exactly once, in order, by chunks of at most `chunk`, none empty
static void check_chunks(int64_t total, int64_t chunk, int64_t want_count) {
  const IdoChunks p(total, chunk);
  std::vector<int> seen((size_t)total, 0);
  int64_t next = 0;
  for (int64_t c = 0; c < p.count(); ++c) {
    CHECK(p.first(c) == next);
    CHECK(p.len(c) >= 1 && p.len(c) <= chunk && p.len(c) <= p.staging());
    for (int64_t o = p.first(c); o < p.first(c) + p.len(c); ++o) {
      CHECK(o >= 0 && o < total);
      if (o >= 0 && o < total) seen[(size_t)o]++;
    }
    next += p.len(c);
  }
  CHECK(next == total);
  for (int64_t o = 0; o < total; ++o) CHECK(seen[(size_t)o] == 1);
  CHECK(p.count() == want_count);
  CHECK(p.staging() == (total < chunk ? total : chunk));
  printf("chunks total %4lld chunk %3lld -> %lld chunks, staging %lld\n", (long long)total, (long long)chunk, (long long)p.count(),
         (long long)p.staging());
}

static void check_range(const char* name, const std::vector<int64_t>& ids, int64_t id_base, int64_t ntotal, int64_t want) {
  const int64_t bad = ido_first_bad(ids.data(), (int64_t)ids.size(), id_base, ntotal);
  printf("range %-34s base %5lld ntotal %4lld -> %lld\n", name, (long long)id_base, (long long)ntotal, (long long)bad);
  CHECK(bad == want);
}

// the route of `ids` over shards [lo, hi) against a per-id linear search; mapped = id + 1000 per shard, put back in request order
static void check_route(const char* name, const std::vector<int64_t>& lo, const std::vector<int64_t>& hi, const std::vector<int64_t>& ids,
                        int64_t want_bad) {
  const int P = (int)lo.size();
  IdoRoute r;
  const int64_t bad = ido_route(ids.data(), (int64_t)ids.size(), lo.data(), hi.data(), P, r);
  printf("route %-34s shards %d ids %3zu -> bad %lld\n", name, P, ids.size(), (long long)bad);
  CHECK(bad == want_bad);
  if (bad >= 0 || want_bad >= 0) return;
  CHECK((int)r.ids.size() == P && (int)r.pos.size() == P);
  size_t routed = 0, minus = 0;
  std::vector<int64_t> out(ids.size(), -7);
  for (size_t i = 0; i < ids.size(); ++i)
    if (ids[i] == -1) out[i] = -1, ++minus;
  for (int g = 0; g < P; ++g) {
    CHECK(r.ids[(size_t)g].size() == r.pos[(size_t)g].size());
    std::vector<int64_t> mapped;
    int64_t last = -1;
    for (size_t j = 0; j < r.ids[(size_t)g].size(); ++j) {
      const int64_t v = r.ids[(size_t)g][j], p = r.pos[(size_t)g][j];
      CHECK(v >= lo[(size_t)g] && v < hi[(size_t)g]);
      CHECK(p > last && p < (int64_t)ids.size() && ids[(size_t)p] == v);  // request order inside a shard
      last = p;
      mapped.push_back(v + 1000 * (g + 1));
    }
    routed += mapped.size();
    ido_scatter_back(r, g, mapped.data(), out.data());
  }
  CHECK(routed + minus == ids.size());
  for (size_t i = 0; i < ids.size(); ++i) {
    if (ids[i] == -1) {
      CHECK(out[i] == -1);
      continue;
    }
    int g = 0;
    while (g < P && !(ids[i] >= lo[(size_t)g] && ids[i] < hi[(size_t)g])) ++g;
    CHECK(g < P && out[i] == ids[i] + 1000 * (g + 1));
  }
}

int main() {
  // dense0 and the searches: empty lists at the front, in a run in the middle, at the end, everywhere at once
  check_dense0("the crafted lists of the GPU test", {0, 1, 31, 32, 33, 0, 0, 65, 0});
  check_dense0("empty at the front", {0, 0, 0, 5, 40});
  check_dense0("a run of empty lists in the middle", {7, 0, 0, 0, 0, 64, 1});
  check_dense0("empty at the end", {33, 2, 0, 0, 0});
  check_dense0("one list", {162});
  check_dense0("one row", {0, 1, 0});
  check_dense0("no empty list, ragged tiles", {1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 97});
  {
    std::vector<unsigned> big(1000);
    for (size_t l = 0; l < big.size(); ++l) big[l] = (unsigned)((l * 2654435761u) % 7 == 0 ? 0 : (l * 40503u) % 90);
    check_dense0("a thousand lists, one in seven empty", big);
  }
  {  // sizes whose sum passes 2^32: the prefix sums are 64-bit
    std::vector<unsigned> huge(5, 0xF0000000u);
    std::vector<int64_t> d0;
    ido_dense0(huge.data(), 5, d0);
    CHECK(d0[5] == (int64_t)5 * 0xF0000000ll);
    printf("dense0 %-34s -> %lld\n", "sizes beyond 2^32 rows", (long long)d0[5]);
  }

  // the chunk plan of the export
  check_chunks(1, 64, 1);
  check_chunks(63, 64, 1);
  check_chunks(64, 64, 1);
  check_chunks(65, 64, 2);
  check_chunks(162, 64, 3);
  check_chunks(0, 64, 0);
  CHECK(ido_chunk_from_env(nullptr) == IDO_CHUNK_DEFAULT && ido_chunk_from_env("") == IDO_CHUNK_DEFAULT);
  CHECK(ido_chunk_from_env("64") == 64 && ido_chunk_from_env("1") == 64 && ido_chunk_from_env("-5") == 64);
  CHECK(ido_chunk_from_env("1000") == 1000 && ido_chunk_from_env("abc") == IDO_CHUNK_DEFAULT);
  CHECK(IDO_CHUNK_DEFAULT == ((int64_t)1 << 22));
  printf("chunks environment values ok\n");

  // the range check
  check_range("all inside, id_base 0", {0, 5, 161, 7, 7}, 0, 162, -1);
  check_range("-1 passes", {-1, 0, -1, 161, -1}, 0, 162, -1);
  check_range("at id_base + ntotal", {0, 161, 162, 200}, 0, 162, 2);
  check_range("below id_base", {1000, 1161, 999}, 1000, 162, 2);
  check_range("at id_base + ntotal, id_base 1000", {1000, 1162}, 1000, 162, 1);
  check_range("-1 with id_base 1000", {-1, 1000, -1}, 1000, 162, -1);
  check_range("-2 is not -1", {5, -2}, 0, 162, 1);
  check_range("0 below id_base 1000", {0}, 1000, 162, 0);
  check_range("INT64_MIN / MAX", {INT64_MAX}, 1000, 162, 0);
  check_range("INT64_MIN", {INT64_MIN}, 1000, 162, 0);
  check_range("nothing to check", {}, 0, 162, -1);

  // shard routing: 1, 2 and 3 shards, both sides of every boundary, duplicates, -1, an id past the last shard
  check_route("one shard", {0}, {100}, {0, 99, 50, 50, -1, 0}, -1);
  check_route("one shard, past the end", {0}, {100}, {0, 99, 100}, 2);
  check_route("two shards, both sides of the cut", {0, 100}, {100, 250}, {99, 100, 0, 249, 99, 100, -1, 101, 98}, -1);
  check_route("two shards, past the last", {0, 100}, {100, 250}, {99, 100, 250}, 2);
  check_route("two shards, below the first", {10, 100}, {100, 250}, {10, 9}, 1);
  check_route("three shards, every boundary", {0, 54, 108}, {54, 108, 162}, {0, 53, 54, 107, 108, 161, 53, 54, -1, -1, 107, 108, 0, 161}, -1);
  check_route("three shards, past the last", {0, 54, 108}, {54, 108, 162}, {161, -1, 162, 0}, 2);
  check_route("three shards, only -1", {0, 54, 108}, {54, 108, 162}, {-1, -1, -1}, -1);
  check_route("three shards, an empty one between", {0, 54, 54}, {54, 54, 162}, {53, 54, 161, 54}, -1);
  check_route("three shards, nothing asked", {0, 54, 108}, {54, 108, 162}, {}, -1);

  if (failures) {
    printf("%d checks FAILED\n", failures);
    return 1;
  }
  printf("id order ok\n");
  return 0;
}
