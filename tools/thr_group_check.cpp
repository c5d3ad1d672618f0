// thr_group_check.cpp -- drives the group driver of the large-k search on a compressed index (clip-retrieval_amd/csrc/knnx_thr_group.h)
// the way knnx_range.hip does, with this program playing the device: no GPU, no HIP, nothing but the header.
// tests/test_ivfpq_threshold_cpu.py builds and runs it.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -I clip-retrieval_amd/csrc tools/thr_group_check.cpp -o thr_group_check      (one command line)
//   ./thr_group_check          (prints one line per case, exit status 0 when every assertion held)
//
// Per query the "device" holds an array of (score, id).  A scan counts the rows with score > thr[i] exactly and collects them into
// the query's slice of `cap` entries -- the first `cap` it meets when there are more, in an arbitrary order.  The host loop around the
// driver is the one of search_large_k_thr_locked: thresholds, scan, absorb, fetch the selected slices packed, take, regrow.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "knnx_thr_group.h"

using knnx::Hit;
using knnx::HitBetter;
using knnx::ThrGroup;

static int g_failed = 0;
#define EXPECT(cond, ...)                   \
  do {                                      \
    if (!(cond)) {                          \
      ++g_failed;                           \
      printf("FAILED %s: ", #cond);         \
      printf(__VA_ARGS__);                  \
      printf("\n");                         \
    }                                       \
  } while (0)

static const int PASS_MAX = 256;  // queries of one pass (PQ_PASS; sq_pass_max at its largest)
static const int NTOP = 64;       // scores of the k = 64 pass
static const int BUDGET = 200;    // scans of one group: a descent ends within 80 (descent_check.cpp), regrows add a few

typedef std::vector<Hit> Rows;  // one query's probed rows, in "arena" order

static std::mt19937 g_rng(11);

// the rows of q above thr into slice (cap entries); returns the exact count
static unsigned scan_query(const Rows& rows, float thr, Hit* slice, unsigned cap, unsigned start) {
  unsigned cnt = 0;
  const size_t T = rows.size();
  for (size_t j = 0; j < T; ++j) {
    const Hit& h = rows[(j + start) % T];  // (an arbitrary order: every scan starts somewhere else)
    if (h.first > thr) {
      if (cnt < cap) slice[cnt] = h;
      ++cnt;
    }
  }
  return cnt;
}

struct Outcome {
  int scans = 0, regrows = 0, mixed_steps = 0, grow_with_fetched = 0;
  size_t pool = 0;
};

// queries: the group; kc: rows wanted; pool: starting entries of the hit pool
static Outcome run_group(const std::string& name, const std::vector<Rows>& queries, int64_t kc, size_t pool) {
  const int gq = (int)queries.size();
  Outcome out;
  std::vector<float> top((size_t)gq * NTOP, -FLT_MAX);
  std::vector<int64_t> total((size_t)gq);
  std::vector<Rows> want((size_t)gq);  // brute force: the first min(kc, total) of a sort by (score descending, id ascending)
  for (int i = 0; i < gq; ++i) {
    want[i] = queries[i];
    std::sort(want[i].begin(), want[i].end(), HitBetter());
    for (size_t j = 0; j < std::min<size_t>(NTOP, want[i].size()); ++j) top[(size_t)i * NTOP + j] = want[i][j].first;
    total[i] = (int64_t)want[i].size();
    if ((int64_t)want[i].size() > kc) want[i].resize((size_t)kc);
  }
  ThrGroup g;
  g.start(gq, kc, top.data(), NTOP, total.data());
  std::vector<float> thr((size_t)gq);
  std::vector<unsigned> counts((size_t)gq);
  std::vector<int> took_part((size_t)gq, 0);  // scans in which the query was not yet fetched
  std::vector<char> fetched((size_t)gq, 0);
  int64_t reported = 0;
  std::vector<Hit> slices;
  std::vector<float> hd;
  std::vector<int64_t> hi;
  while (g.left > 0 && out.scans < BUDGET) {
    const unsigned cap = (unsigned)std::min<size_t>(pool / (size_t)gq, 0xffffffffu);
    g.thresholds(thr.data());
    slices.assign((size_t)gq * cap + 1, Hit(0.f, -7));
    int descending = 0, finals = 0;
    for (int i = 0; i < gq; ++i) {
      if (fetched[i]) {
        EXPECT(thr[i] == INFINITY, "%s: query %d was fetched and is scanned again at %g", name.c_str(), i, thr[i]);
      } else {
        EXPECT(thr[i] < INFINITY && thr[i] == thr[i], "%s: query %d threshold %g", name.c_str(), i, thr[i]);
        ++took_part[i];
      }
      counts[i] = scan_query(queries[i], thr[i], slices.data() + (size_t)i * cap, cap, (unsigned)g_rng());
      if (fetched[i]) EXPECT(counts[i] == 0, "%s: +INFINITY let %u rows through", name.c_str(), counts[i]);
    }
    ++out.scans;
    const ThrGroup::Step s = g.absorb(counts.data(), cap);
    reported += s.query_scans;
    // what the step says must hang together
    int64_t nsel = 0;
    unsigned grow = 0;
    for (int i = 0; i < gq; ++i) {
      nsel += g.sel[i];
      if (fetched[i]) EXPECT(g.sel[i] == 0 && !g.picked[i], "%s: query %d selected twice", name.c_str(), i);
      if (g.picked[i]) EXPECT(g.sel[i] == counts[i] && counts[i] <= cap, "%s: query %d sel %u count %u cap %u", name.c_str(), i, g.sel[i], counts[i], cap);
      if (!g.picked[i]) EXPECT(g.sel[i] == 0, "%s: query %d not picked but sel %u", name.c_str(), i, g.sel[i]);
      if (!fetched[i] && g.state[i] == ThrGroup::FINAL && !g.picked[i]) grow = std::max(grow, counts[i]);
      if (!fetched[i] && g.state[i] == ThrGroup::DESCENDING) ++descending;
      if (!fetched[i] && g.state[i] == ThrGroup::FINAL) ++finals;
    }
    EXPECT(nsel == s.nsel, "%s: nsel %lld, sum of sel %lld", name.c_str(), (long long)s.nsel, (long long)nsel);
    EXPECT(grow == s.grow, "%s: grow %u, expected %u", name.c_str(), s.grow, grow);
    if (s.grow) EXPECT(s.grow > cap, "%s: grow %u fits cap %u", name.c_str(), s.grow, cap);
    if (descending && finals) ++out.mixed_steps;
    // the fetch: the selected slices packed in query order
    hd.clear();
    hi.clear();
    for (int i = 0; i < gq; ++i)
      for (unsigned j = 0; j < g.sel[i]; ++j) {
        hd.push_back(slices[(size_t)i * cap + j].first);
        hi.push_back(slices[(size_t)i * cap + j].second);
      }
    const int left_before = g.left;
    int picked = 0;
    for (int i = 0; i < gq; ++i) picked += g.picked[i] ? 1 : 0;
    g.take(hd.data(), hi.data());
    EXPECT(g.left == left_before - picked, "%s: left %d -> %d with %d queries taken", name.c_str(), left_before, g.left, picked);
    for (int i = 0; i < gq; ++i)
      if (g.state[i] == ThrGroup::FETCHED) fetched[i] = 1;
    if (s.grow) {
      int nf = 0;
      for (int i = 0; i < gq; ++i) nf += fetched[i];
      if (nf) ++out.grow_with_fetched;
      const size_t w = knnx::pool_want(pool, (size_t)gq, s.grow);
      EXPECT(w / (size_t)gq >= s.grow && w > pool, "%s: pool %zu -> %zu does not fit %u x %d", name.c_str(), pool, w, s.grow, gq);
      pool = w;
      ++out.regrows;
    }
  }
  EXPECT(g.left == 0, "%s: %d queries not fetched after %d scans", name.c_str(), g.left, out.scans);
  int64_t expected_part = 0;
  for (int i = 0; i < gq; ++i) {
    expected_part += took_part[i];
    EXPECT(g.state[i] == ThrGroup::FETCHED, "%s: query %d ends in state %d", name.c_str(), i, (int)g.state[i]);
    const Rows& h = g.hits[i];
    bool same = h.size() == want[i].size();
    for (size_t j = 0; same && j < h.size(); ++j) same = h[j].first == want[i][j].first && h[j].second == want[i][j].second;
    EXPECT(same, "%s: query %d: %zu hits, brute force %zu (or another order)", name.c_str(), i, h.size(), want[i].size());
  }
  EXPECT(reported == expected_part, "%s: %lld participations reported, %lld counted", name.c_str(), (long long)reported, (long long)expected_part);
  out.pool = pool;
  printf("%-44s gq %3d  kc %6lld  scans %3d  regrows %d  mixed steps %d  final pool %zu\n", name.c_str(), gq, (long long)kc, out.scans, out.regrows,
         out.mixed_steps, pool);
  return out;
}

// ---- score arrays ------------------------------------------------------------------------------------------------------------
static Rows with_ids(const std::vector<float>& s, int64_t id0) {
  Rows r(s.size());
  std::vector<int64_t> ids(s.size());
  for (size_t j = 0; j < s.size(); ++j) ids[j] = id0 + (int64_t)j;
  std::shuffle(ids.begin(), ids.end(), g_rng);  // ids in no relation to the scores or the arena order
  for (size_t j = 0; j < s.size(); ++j) r[j] = Hit(s[j], ids[j]);
  return r;
}
static Rows bell(size_t n) {
  std::normal_distribution<float> d(0.f, 0.05f);
  std::vector<float> s(n);
  for (float& v : s) v = d(g_rng);
  return with_ids(s, 1000);
}
static Rows uniform(size_t n) {
  std::uniform_real_distribution<float> d(-0.2f, 0.6f);
  std::vector<float> s(n);
  for (float& v : s) v = d(g_rng);
  return with_ids(s, 0);
}
// 64 near-duplicates far above everything else: the local density says nothing about the rest, the descent needs several steps
static Rows gap_then_crowd(size_t n) {
  std::normal_distribution<float> d(0.f, 0.03f);
  std::vector<float> s(n);
  for (float& v : s) v = d(g_rng);
  for (size_t j = 0; j < 64 && j < n; ++j) s[j] = 0.9f + 1e-6f * (float)j;
  return with_ids(s, 300);
}
static Rows all_equal(size_t n) { return with_ids(std::vector<float>(n, 0.25f), 5); }
// few distinct scores: whole plateaus of exact ties, one of them across the kc-th place
static Rows tied(size_t n, int levels) {
  std::uniform_int_distribution<int> d(0, levels - 1);
  std::vector<float> s(n);
  for (float& v : s) v = 0.5f - 0.01f * (float)d(g_rng);
  return with_ids(s, 77);
}

static void check_pool_want() {
  const size_t pools[] = {1, 2, 3, 64, 1000, (size_t)1 << 21};
  const size_t slices[] = {1, 2, 7, 32, 255, 256};
  const size_t mxs[] = {0, 1, 2, 5, 63, 64, 65, 4097, 100000, 0xffffffffu};
  int n = 0;
  for (size_t p : pools)
    for (size_t sl : slices)
      for (size_t mx : mxs) {
        const size_t w = knnx::pool_want(p, sl, mx);
        EXPECT(w / sl >= mx, "pool_want(%zu, %zu, %zu) = %zu is too small", p, sl, mx, w);
        size_t shift = 0;
        while ((p << shift) < w) ++shift;
        EXPECT((p << shift) == w, "pool_want(%zu, %zu, %zu) = %zu is no doubling of the pool", p, sl, mx, w);
        if (w > p) EXPECT((w >> 1) / sl < mx, "pool_want(%zu, %zu, %zu) = %zu: half of it fits already", p, sl, mx, w);
        ++n;
      }
  printf("%-44s %d combinations\n", "pool_want", n);
}

static void check_rank_and_write() {
  Rows h = {Hit(0.5f, 9), Hit(0.7f, 3), Hit(0.5f, 2), Hit(0.5f, 4), Hit(-1.f, 0)};
  Rows a = h;
  knnx::rank_hits(a, 3);  // the tie at 0.5 across the third place: the smaller id wins
  EXPECT(a.size() == 3 && a[0] == Hit(0.7f, 3) && a[1] == Hit(0.5f, 2) && a[2] == Hit(0.5f, 4), "rank_hits keep 3");
  Rows b = h;
  knnx::rank_hits(b, 10);
  EXPECT(b.size() == 5 && b[4] == Hit(-1.f, 0) && b[3] == Hit(0.5f, 9), "rank_hits keep 10");
  float D[4];
  int64_t I[4];
  knnx::write_topk(a, 2, D, I);
  EXPECT(D[0] == 0.7f && I[0] == 3 && D[1] == 0.5f && I[1] == 2, "write_topk truncates");
  knnx::write_topk(a, 4, D, I);
  EXPECT(D[2] == 0.5f && I[2] == 4 && D[3] == -FLT_MAX && I[3] == -1, "write_topk pads");
  knnx::write_topk(Rows(), 1, D, I);
  EXPECT(D[0] == -FLT_MAX && I[0] == -1, "write_topk of nothing");
  printf("%-44s ok\n", "rank_hits / write_topk");
}

int main() {
  check_pool_want();
  check_rank_and_write();
  const size_t POOL0 = (size_t)1 << 21;  // what range_pool_slice starts with

  // one shape at a time, a few queries each
  run_group("bell", {bell(20000), bell(30000), bell(9000)}, 100, POOL0);
  run_group("uniform", {uniform(20000), uniform(700)}, 100, POOL0);
  run_group("all equal", {all_equal(5000), all_equal(300)}, 100, POOL0);
  run_group("ties across the kc-th place", {tied(6000, 40), tied(6000, 3), tied(500, 2)}, 100, POOL0);
  run_group("total <= 2 kc: one scan", {bell(200), uniform(101), all_equal(199)}, 100, POOL0);
  {
    const Outcome o = run_group("total <= 2 kc alone", {bell(200), bell(150)}, 100, POOL0);
    EXPECT(o.scans == 1, "total <= 2 kc took %d scans", o.scans);
  }
  run_group("total < kc and total = 0", {bell(99), uniform(1), Rows(), bell(64), bell(63)}, 100, POOL0);
  run_group("total = 0 alone", {Rows()}, 100, POOL0);
  run_group("kc = 65", {bell(20000), uniform(5000), all_equal(130), all_equal(131), tied(3000, 5), Rows()}, 65, POOL0);
  run_group("kc = 3000", {bell(60000), uniform(40000), all_equal(6001), tied(20000, 30), bell(2999), bell(3000), bell(6000)}, 3000, POOL0);

  // a query that is final while another one still descends: the small one takes everything in scan 1, the bell needs several
  {
    const Outcome o = run_group("final next to descending", {bell(150), gap_then_crowd(50000), all_equal(100)}, 100, POOL0);
    EXPECT(o.scans > 1 && o.mixed_steps >= 1, "scans %d, steps with a final query next to a descending one %d", o.scans, o.mixed_steps);
  }
  // the same with a query that is final but does NOT fit while others descend or are fetched: a pool of 4 entries per query
  {
    std::vector<Rows> qs = {bell(150), gap_then_crowd(30000), all_equal(100), Rows(), uniform(4000), bell(3)};
    const Outcome o = run_group("tiny pool: grow next to fetched queries", qs, 100, 4 * qs.size());
    EXPECT(o.regrows >= 1 && o.grow_with_fetched >= 1, "regrows %d, with fetched queries %d", o.regrows, o.grow_with_fetched);
  }
  {
    std::vector<Rows> qs = {all_equal(5000), bell(40000), tied(8000, 4)};
    const Outcome o = run_group("tiny pool: all-equal overflows", qs, 1000, 64);
    EXPECT(o.regrows >= 1, "regrows %d", o.regrows);
  }
  // a pool smaller than the group: every slice has cap = 0 until it has grown
  {
    std::vector<Rows> qs = {bell(500), Rows(), bell(100), uniform(64)};
    const Outcome o = run_group("pool smaller than the group (cap 0)", qs, 65, 2);
    EXPECT(o.regrows >= 1, "regrows %d", o.regrows);
  }

  // a full pass of mixed queries
  {
    std::vector<Rows> qs;
    std::uniform_int_distribution<int> kind(0, 6), size(0, 4000);
    for (int i = 0; i < PASS_MAX; ++i) {
      const size_t n = (size_t)size(g_rng);
      switch (kind(g_rng)) {
        case 0: qs.push_back(gap_then_crowd(n + 3000)); break;
        case 1: qs.push_back(uniform(n)); break;
        case 2: qs.push_back(all_equal(n / 4)); break;
        case 3: qs.push_back(tied(n, 7)); break;
        case 4: qs.push_back(bell(n % 150)); break;
        case 5: qs.push_back(Rows()); break;
        default: qs.push_back(bell(n)); break;
      }
    }
    const Outcome a = run_group("a full pass, mixed", qs, 100, POOL0);
    EXPECT(a.mixed_steps >= 1, "no step had a final query next to a descending one");
    const Outcome b = run_group("a full pass, mixed, tiny pool", qs, 300, 16 * (size_t)PASS_MAX);
    EXPECT(b.regrows >= 1 && b.grow_with_fetched >= 1, "regrows %d, with fetched queries %d", b.regrows, b.grow_with_fetched);
  }

  if (g_failed) {
    printf("%d assertion(s) failed\n", g_failed);
    return 1;
  }
  printf("thr group ok\n");
  return 0;
}
