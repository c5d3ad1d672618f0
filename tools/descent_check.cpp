// descent_check.cpp -- drives the threshold descent of the IVF-PQ large-k search (clip-retrieval_amd/csrc/knnx_descent.h) against
// synthetic score arrays on the host: no GPU, no HIP, nothing but the header.  tests/test_ivfpq_threshold_cpu.py builds and runs it.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -I clip-retrieval_amd/csrc tools/descent_check.cpp -o descent_check
//   ./descent_check            (prints one line per case, exit status 0 when every assertion held)
//
// A "scan" here is what pq_range_scan_kernel computes for one query: the number of scores strictly above the threshold.  For every
// case the program asserts that the descent ends within a fixed budget of scans, that the scan it fetches holds at least
// min(k, T) rows, and that it never fetches more than 16 k rows (when that is more than 65 536) once a scan with a count in
// [min(k, T), 16 k] has been seen.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "knnx_descent.h"

using knnx::PqDescent;

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

// scores sorted descending; rows strictly above thr
static int64_t count_above(const std::vector<float>& s, float thr) {
  return std::upper_bound(s.begin(), s.end(), thr, std::greater<float>()) - s.begin();
}

static const int BUDGET = 80;  // 60 doublings + 4 bisections + their steps back + the take-everything scan, with room

// s: sorted descending
static void run_case(const std::string& name, const std::vector<float>& s, int64_t k) {
  const int64_t T = (int64_t)s.size();
  const float s32 = T >= 32 ? s[31] : -FLT_MAX, s64 = T >= 64 ? s[63] : -FLT_MAX;
  const int64_t want = std::min(k, T);
  PqDescent d;
  d.start(s32, s64, k, T);
  EXPECT(d.want == want, "%s: want %lld", name.c_str(), (long long)d.want);
  if (T <= 2 * k) EXPECT(d.thr == -FLT_MAX, "%s: T <= 2 k must take everything in one scan", name.c_str());
  int scans = 0;
  bool feasible_seen = false;  // a scan with want <= count <= 16 k
  int64_t cnt = 0;
  for (;;) {
    EXPECT(d.thr != INFINITY && d.thr == d.thr, "%s: threshold %g", name.c_str(), d.thr);
    cnt = count_above(s, d.thr);
    ++scans;
    if (cnt >= want && cnt <= 16 * k) feasible_seen = true;
    if (scans > BUDGET) break;
    if (d.next(cnt) == PqDescent::FETCH) break;
  }
  EXPECT(scans <= BUDGET, "%s: no end after %d scans", name.c_str(), scans);
  EXPECT(scans == d.scans, "%s: the descent counted %d scans, the driver %d", name.c_str(), d.scans, scans);
  EXPECT(cnt >= want, "%s: fetched %lld of %lld wanted rows", name.c_str(), (long long)cnt, (long long)want);
  if (feasible_seen)
    EXPECT(cnt <= 16 * k || cnt <= PqDescent::OVERSHOOT_MIN, "%s: fetched %lld rows after a scan within 16 k = %lld had been seen",
           name.c_str(), (long long)cnt, (long long)(16 * k));
  if (T <= 2 * k) EXPECT(scans == 1, "%s: %d scans where one takes everything", name.c_str(), scans);
  printf("%-34s T %8lld  k %7lld  scans %2d  fetched %8lld  bisections %d\n", name.c_str(), (long long)T, (long long)k, scans, (long long)cnt,
         d.bisections);
}

static std::vector<float> sorted(std::vector<float> s) {
  std::sort(s.begin(), s.end(), std::greater<float>());
  return s;
}

int main() {
  std::mt19937 rng(7);
  auto fill = [&](size_t n, auto dist) {
    std::vector<float> s(n);
    for (float& v : s) v = dist(rng);
    return s;
  };
  std::vector<std::pair<std::string, std::vector<float>>> cases;
  // uniform scores
  for (size_t T : {(size_t)200, (size_t)5000, (size_t)400000})
    cases.emplace_back("uniform", sorted(fill(T, std::uniform_real_distribution<float>(-0.2f, 0.6f))));
  // a bell of scores (what inner products of unit vectors look like): dense far below the top
  cases.emplace_back("normal", sorted(fill(400000, std::normal_distribution<float>(0.f, 0.05f))));
  // one very close neighbour, then a gap, then the crowd: s32 - s64 is tiny next to top - s64
  {
    std::vector<float> s = fill(400000, std::normal_distribution<float>(0.f, 0.04f));
    s[0] = 0.99f;
    cases.emplace_back("one close neighbour, then a gap", sorted(s));
  }
  // 64 near-duplicates far above everything else: the local density says nothing about the rest
  {
    std::vector<float> s = fill(300000, std::normal_distribution<float>(0.f, 0.03f));
    for (int i = 0; i < 64; ++i) s[(size_t)i] = 0.9f + 1e-6f * (float)i;
    cases.emplace_back("64 near-duplicates, then a gap", sorted(s));
  }
  cases.emplace_back("all equal (small)", std::vector<float>(5000, 0.25f));
  cases.emplace_back("all equal (large)", std::vector<float>(400000, 0.25f));
  cases.emplace_back("T = 0", std::vector<float>());
  // huge magnitudes: steps and thresholds must not overflow
  cases.emplace_back("huge negative", sorted(fill(200000, std::uniform_real_distribution<float>(-3e37f, -1e37f))));
  const int64_t ks[] = {65, 100, 1000, 3000, 100000};
  for (int64_t k : ks) {
    for (const auto& c : cases) run_case(c.first, c.second, k);
    // fewer rows than k
    run_case("T < k (all equal)", std::vector<float>((size_t)std::min<int64_t>(k - 1, 40000), 0.1f), k);
    run_case("T < k (uniform)", sorted(fill((size_t)std::min<int64_t>(k / 2 + 3, 50000), std::uniform_real_distribution<float>(-1.f, 1.f))), k);
  }
  if (g_failed) {
    printf("%d assertion(s) failed\n", g_failed);
    return 1;
  }
  printf("descent ok\n");
  return 0;
}
