// gemm_plan_check.cpp -- drives csrc/clipx_gemm_plan.h (which kernels one launch_gemm call runs, on which rows) on the CPU.  Its own
// main, only that header: built with -fsanitize=address,undefined by tests/test_gemm_plan_cpu.py and run as a child process.
//   g++ -std=c++17 -O2 -g -fsanitize=address,undefined -pthread -I clip-retrieval_amd/csrc tools/gemm_plan_check.cpp -o gemm_plan_check
// Every case demands what the code the plan replaced gave -- the four gemm256_* functions, splitk_factor, the two predicates of
// the 4-wave kernel and the branches of launch_gemm / launch_gemm128 / launch_gemm_epi reduced to "the list of launches", all
// restated below as they were -- and the properties a plan must have.  The sweep is a full cross product (see main).
// Prints nothing unless a check fails, then the case count, how many swept shapes put more tail strips into a launch than it has
// workgroups that own a bulk tile (a figure, not a failure), and "gemm plan ok"; a failed check prints FAILED, exit status 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

#include "clipx_gemm_plan.h"

using namespace clipx;

// ---------------------------------------------------------------------------------------------------------------------------
// the code as it was
// ---------------------------------------------------------------------------------------------------------------------------
namespace old {

struct Args {
  int M, N, K, epi, variant, n_cu, row0, f16;
  bool rowstats;  // stats_eps > 0
  bool splitk_ws;
  size_t splitk_ws_bytes;
  int tail_m0, tail_nb;
};

constexpr int G_TM = 128, G_TN = 128, G_BK = 64;

static int splitk_factor(const Args& g) {
  if (!g.splitk_ws || g.M > 1024 || g.epi == EPI_TABLE_F32 || g.epi == EPI_RAW_F32) return 1;
  const int nk = g.K / G_BK;
  if (nk < 8 || (nk < 32 && g.M > G_TM)) return 1;
  const int cu = g.n_cu > 0 ? g.n_cu : 256;
  const int tiles = ((g.M + G_TM - 1) / G_TM) * (g.N / G_TN);
  int S = 1;
  for (int c = 2; c <= 16; ++c) {
    if (nk % c != 0 || nk / c < 4) continue;
    if ((size_t)c * g.M * g.N * sizeof(float) > g.splitk_ws_bytes) break;
    if (tiles * (c - 1) >= cu) break;
    S = c;
  }
  return S;
}

static int gemm256_bulk_mtiles(int M, int N, int n_cu) {
  const int mt = M / 256, nt = N / 256;
  if (mt <= 0 || nt <= 0) return 0;
  const int cu = (n_cu > 0 ? n_cu : 256) & ~7;
  int best = mt;
  double best_cost = 1e30;
  for (int peel = 0; peel <= 8 && peel < mt; ++peel) {
    const int bulk = mt - peel;
    const int rounds = (bulk * nt + cu - 1) / cu;
    const double rest = (double)(peel * 4 * nt) / (2.0 * cu);
    const double cost = rounds + (peel ? 0.25 * (rest > 1.0 ? rest : 1.0) / 0.6 : 0.0);
    if (cost < best_cost - 1e-9) { best_cost = cost; best = bulk; }
  }
  return best;
}

static int gemm256_tail_blocks(int N, int K, int n_cu) {
  int grid = (n_cu > 0 ? n_cu : 256) & ~7;
  if (grid < 8) grid = 8;
  if (N % 32 || K % 128 || (size_t)32 * K * 2 >= ((size_t)1 << 31)) return 0;
  const int cb = N / 32;
  for (int nb = 1; nb <= 4; ++nb)
    if (cb % nb == 0 && 8 * (cb / nb) <= grid) return nb;
  return 0;
}

static int gemm256_dispatch_mtiles(int M, int N, int K, int variant, int n_cu) {
  if (variant < 2 || N % 256 != 0 || K % 128 != 0 || M < 256) return 0;
  const int bulk = gemm256_bulk_mtiles(M, N, n_cu);
  const int cu = (n_cu > 0 ? n_cu : 256);
  return bulk > 0 && (int64_t)bulk * (N / 256) >= cu / 2 ? bulk : 0;
}

static int gemm256_whole_tile_rows(int M, int N, int K, int variant, int n_cu) {
  const int Mp = (M + 255) / 256 * 256;
  return Mp != M && gemm256_dispatch_mtiles(Mp, N, K, variant, n_cu) > 0 ? Mp : M;
}

static bool gemm256w4_supports(const Args& g) {
  if (g.M <= 0 || g.M % 256 != 0 || g.N % 256 != 0 || g.K % 128 != 0 || g.K < 256) return false;
  if (g.f16) return g.epi == EPI_BIAS_BF16 || g.epi == EPI_BIAS_F16 || g.epi == EPI_BIAS_QGELU_BF16 || g.epi == EPI_BIAS_GELU_BF16;
  return g.epi == EPI_BIAS_BF16 || g.epi == EPI_BIAS_F16 || g.epi == EPI_BIAS_QGELU_BF16 || g.epi == EPI_BIAS_GELU_BF16 || g.epi == EPI_BIAS_RESID_H16;
}
static bool gemm256w4_fuses_stats(const Args& g) {
  return g.rowstats && g.f16 && gemm256w4_supports(g) &&
         (g.epi == EPI_BIAS_BF16 || g.epi == EPI_BIAS_F16 || g.epi == EPI_BIAS_QGELU_BF16 || g.epi == EPI_BIAS_GELU_BF16);
}

}  // namespace old

// one launch: what, first row, rows, and two details (W4 / W8: tail_nb and "takes the statistics", SPLITK: S, G128: the fill form)
enum { L_ROWSTATS = 1, L_W4, L_W8, L_SPLITK, L_G128 };
struct Launch {
  int kind, first, rows, a, b;
  bool operator==(const Launch& o) const { return kind == o.kind && first == o.first && rows == o.rows && a == o.a && b == o.b; }
};
struct List {
  Launch l[4];
  int n = 0;
  void add(int kind, int first, int rows, int a = 0, int b = 0) { l[n++] = Launch{kind, first, rows, a, b}; }
};

namespace old {

static bool is_one_of(int epi, std::initializer_list<int> set) {
  for (int e : set)
    if (e == epi) return true;
  return false;
}

// launch_gemm128 + launch_gemm_epi + launch_splitk_epi: false = hipErrorInvalidValue
static bool launch_gemm128(const Args& g, int first, List& out) {
  const bool small_off = (size_t)g.M * g.K * 2 < ((size_t)1 << 32) && (size_t)g.N * g.K * 2 < ((size_t)1 << 32);
  const int S = (g.variant == 1 && small_off) ? splitk_factor(g) : 1;
  if (S > 1 && is_one_of(g.epi, {EPI_BIAS_BF16, EPI_BIAS_F16, EPI_BIAS_QGELU_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_RESID_F32, EPI_BIAS_RESID_H16})) {
    out.add(L_SPLITK, first, g.M, S);
    return true;
  }
  if (g.f16) {
    if (!is_one_of(g.epi, {EPI_BIAS_BF16, EPI_BIAS_F16, EPI_BIAS_QGELU_BF16, EPI_BIAS_GELU_BF16})) return false;
  } else if (!is_one_of(g.epi, {EPI_BIAS_BF16, EPI_BIAS_F16, EPI_BIAS_QGELU_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_RESID_F32, EPI_BIAS_RESID_H16, EPI_TABLE_F32}))
    return false;
  if (g.variant == 1 && g.K >= 2 * G_BK && small_off) out.add(L_G128, first, g.M, GEMM128_DMA_DEEP);
  else if (g.variant == 1) out.add(L_G128, first, g.M, GEMM128_DMA);
  else out.add(L_G128, first, g.M, GEMM128_REG);
  return true;
}
static bool launch_gemm256sp(const Args& g, List& out) {
  if (g.M <= 0 || g.M % 256 != 0 || g.N % 256 != 0 || g.K % 128 != 0 || g.K <= 0) return false;
  if (g.f16) {
    if (!is_one_of(g.epi, {EPI_BIAS_BF16, EPI_BIAS_F16, EPI_BIAS_QGELU_BF16, EPI_BIAS_GELU_BF16})) return false;
  } else if (!is_one_of(g.epi, {EPI_BIAS_BF16, EPI_BIAS_F16, EPI_BIAS_QGELU_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_RESID_F32, EPI_BIAS_RESID_H16, EPI_TABLE_F32}))
    return false;
  out.add(L_W8, 0, g.M, g.tail_nb);
  return true;
}
static bool launch_gemm256w4(const Args& g, List& out) {
  if (!gemm256w4_supports(g)) return false;
  out.add(L_W4, 0, g.M, g.tail_nb, gemm256w4_fuses_stats(g) ? 1 : 0);
  return true;
}

// launch_gemm (without the rowscale pointer check of the 16-bit-output epilogues, which is not the plan's: the sweep always brings one)
static bool launch_gemm(const Args& g0, List& out) {
  Args g = g0;
  if (g.M <= 0 || g.N % G_TN != 0 || g.K % G_BK != 0 || g.K <= 0) return false;
  const bool out16 = g.epi == EPI_BIAS_BF16 || g.epi == EPI_BIAS_QGELU_BF16 || g.epi == EPI_BIAS_GELU_BF16 || g.epi == EPI_BIAS_F16;
  if (g.f16 && !out16) return false;
  if (g.rowstats) {
    if (!g.f16 || !out16) return false;
    int fused_rows = 0;
    if (g.variant == 6 && g.N % 256 == 0 && g.K % 128 == 0 && g.M >= 256) {
      const int bulk = gemm256_bulk_mtiles(g.M, g.N, g.n_cu);
      const int cu = (g.n_cu > 0 ? g.n_cu : 256);
      Args b = g;
      b.M = bulk * 256;
      if (bulk > 0 && (int64_t)bulk * (g.N / 256) >= cu / 2 && gemm256w4_fuses_stats(b)) fused_rows = b.M;
    }
    if (fused_rows < g.M) out.add(L_ROWSTATS, fused_rows, g.M - fused_rows);
    if (fused_rows == 0) g.rowstats = false;
  }
  {
    const int bulk = gemm256_dispatch_mtiles(g.M, g.N, g.K, g.variant, g.n_cu);
    if (bulk > 0) {
      Args b = g;
      b.M = bulk * 256;
      b.tail_m0 = b.tail_nb = 0;
      if (g.M - b.M == 256 && (g.variant == 3 || g.variant == 6) && g.row0 == 0) {
        b.tail_nb = gemm256_tail_blocks(g.N, g.K, g.n_cu);
        b.tail_m0 = b.M;
      }
      const bool tail_inside = b.tail_nb > 0;
      const bool ok = (g.variant == 6 && gemm256w4_supports(b)) ? launch_gemm256w4(b, out) : launch_gemm256sp(b, out);
      if (!ok) return false;
      if (b.M == g.M || tail_inside) return true;
      Args r = g;
      r.variant = 1;
      r.rowstats = false;
      r.splitk_ws = false;
      r.M = g.M - b.M;
      return launch_gemm128(r, b.M, out);
    }
  }
  Args r = g;
  if (r.variant >= 2) r.variant = 1;
  r.rowstats = false;
  return launch_gemm128(r, 0, out);
}

}  // namespace old

// the launches launch_gemm issues from a plan, in its order
static void launches_of(const GemmPlan& p, int M, List& out) {
  if (p.stats_rows > 0) out.add(L_ROWSTATS, p.fused_rows, p.stats_rows);
  if (p.kernel256 == GEMM256_W4) out.add(L_W4, 0, p.rows256, p.tail_nb, p.fused_rows > 0 ? 1 : 0);
  if (p.kernel256 == GEMM256_W8) out.add(L_W8, 0, p.rows256, p.tail_nb);
  if (p.rows128 > 0) {
    if (p.splitk > 1) out.add(L_SPLITK, M - p.rows128, p.rows128, p.splitk);
    else out.add(L_G128, M - p.rows128, p.rows128, p.fill128);
  }
}

struct Tally {
  long cases = 0, failures = 0, valid = 0, strips_over_bulk = 0;
};
static std::mutex print_lock;

#define CHECK(cond)                                                                                                            \
  do {                                                                                                                         \
    if (!(cond)) {                                                                                                             \
      if (t.failures < 10) {                                                                                                   \
        std::lock_guard<std::mutex> lk(print_lock);                                                                            \
        printf("FAILED %s:%d: %s (M %d N %d K %d epi %d f16 %d variant %d n_cu %d row0 %d stats %d ws %zu)\n", __FILE__, __LINE__, #cond, \
               M, N, K, epi, f16, variant, n_cu, row0, (int)stats, ws);                                                        \
      }                                                                                                                        \
      ++t.failures;                                                                                                            \
    }                                                                                                                          \
  } while (0)

static void check_case(Tally& t, int M, int N, int K, int epi, int f16, int variant, int n_cu, int row0, bool stats, size_t ws) {
  ++t.cases;
  old::Args g{M, N, K, epi, variant, n_cu, row0, f16, stats, ws != 0, ws, 0, 0};
  List was, now;
  const bool was_valid = old::launch_gemm(g, was);
  const GemmPlan p = gemm_plan(M, N, K, epi, f16 != 0, variant, n_cu, row0, stats, ws);
  CHECK(p.valid == was_valid);
  if (!p.valid || !was_valid) return;
  ++t.valid;
  launches_of(p, M, now);
  CHECK(now.n == was.n);
  for (int i = 0; i < now.n && i < was.n; ++i) CHECK(now.l[i] == was.l[i]);
  // the row ranges partition [0, M)
  const int tail_rows = p.tail_nb > 0 ? G256_T : 0;
  CHECK(p.rows256 >= 0 && p.rows128 >= 0 && p.rows256 + tail_rows + p.rows128 == M);
  CHECK(p.rows256 % G256_T == 0 && (p.rows256 > 0) == (p.kernel256 != GEMM256_NONE) && (p.rows128 > 0) == (p.fill128 != GEMM128_NONE));
  CHECK(p.bulk_tiles == (p.rows256 / G256_T) * (N / G256_T) && (p.rows256 == 0 || p.grid256 == gemm256_grid(n_cu)));
  CHECK(p.splitk >= 1 && p.splitk <= SPLITK_MAX && (p.splitk == 1 || (p.rows256 == 0 && ws >= (size_t)p.splitk * M * N * sizeof(float))));
  if (p.tail_nb > 0) {  // 1 .. 4 column blocks, a divisor of N / 32; the strips fit the grid
    CHECK(p.tail_nb >= 1 && p.tail_nb <= G256_STRIP_NB_MAX && (N / G256_STRIP) % p.tail_nb == 0 && p.rows256 > 0);
    CHECK(p.tail_strips == G256_STRIP_ROWS * (N / G256_STRIP / p.tail_nb) && p.tail_strips <= p.grid256);
    const int owners = p.bulk_tiles < p.grid256 ? p.bulk_tiles : p.grid256;  // workgroups that own a bulk tile
    if (p.tail_strips > owners) ++t.strips_over_bulk;
  } else {
    CHECK(p.tail_strips == 0);
  }
  // statistics: the rows the 4-wave kernel takes plus the rows of the pass are all rows
  if (stats) CHECK(p.fused_rows + p.stats_rows == M && (p.fused_rows == 0 || (p.fused_rows == p.rows256 && p.kernel256 == GEMM256_W4)));
  else CHECK(p.fused_rows == 0 && p.stats_rows == 0);
}

// the functions callers use on their own, against the code as it was
static void check_functions(Tally& t, int M, int N, int K, int n_cu) {
  const int epi = -1, f16 = -1, variant = -1, row0 = -1;
  const bool stats = false;
  const size_t ws = 0;
  CHECK(gemm256_bulk_mtiles(M, N, n_cu) == old::gemm256_bulk_mtiles(M, N, n_cu));
  CHECK(gemm256_tail_blocks(N, K, n_cu) == old::gemm256_tail_blocks(N, K, n_cu));
  for (int v = 0; v <= GEMM_V_MAX; ++v) {
    CHECK(gemm256_dispatch_mtiles(M, N, K, v, n_cu) == old::gemm256_dispatch_mtiles(M, N, K, v, n_cu));
    CHECK(gemm256_whole_tile_rows(M, N, K, v, n_cu) == old::gemm256_whole_tile_rows(M, N, K, v, n_cu));
  }
  for (int e = 0; e < 8; ++e)
    for (int h = 0; h < 2; ++h) {
      old::Args g{M, N, K, e, 6, n_cu, 0, h, true, false, 0, 0, 0};
      CHECK(gemm256w4_supports(M, N, K, e, h != 0) == old::gemm256w4_supports(g));
      CHECK(gemm256w4_fuses_stats(M, N, K, e, h != 0) == old::gemm256w4_fuses_stats(g));
      for (size_t bytes : {(size_t)0, (size_t)1 << 20, (size_t)1 << 30}) {
        g.splitk_ws = bytes != 0, g.splitk_ws_bytes = bytes;
        CHECK(gemm_splitk_factor(M, N, K, e, n_cu, bytes) == old::splitk_factor(g));
      }
    }
}

int main() {
  // M: every value 1 .. 600, every multiple of 256 up to 66 048 with its neighbours, 10 547 (41 x 257 + 10: a ragged ViT-L/14 batch)
  // and 65 792 (256 x 257)
  std::set<int> ms;
  for (int m = 1; m <= 600; ++m) ms.insert(m);
  for (int m = 256; m <= 66048; m += 256) ms.insert(m - 1), ms.insert(m), ms.insert(m + 1);
  ms.insert(10547), ms.insert(65792);
  const std::vector<int> Ms(ms.begin(), ms.end());
  const int Ns[] = {128 * 1, 128 * 4, 128 * 6, 128 * 8, 128 * 10, 128 * 18, 128 * 24, 128 * 30, 128 * 32, 128 * 40};
  const int Ks[] = {64, 128, 192, 256, 768, 1024, 1280, 4096};
  const int CUs[] = {0, 8, 64, 256, 304};
  const size_t WSs[] = {0, (size_t)1 << 20, (size_t)1 << 30};

  unsigned nthreads = std::thread::hardware_concurrency();
  nthreads = nthreads < 1 ? 1 : (nthreads > 16 ? 16 : nthreads);
  std::vector<Tally> tallies(nthreads);
  std::atomic<size_t> next{0};
  std::vector<std::thread> pool;
  for (unsigned ti = 0; ti < nthreads; ++ti)
    pool.emplace_back([&, ti] {
      Tally& t = tallies[ti];
      for (size_t i = next++; i < Ms.size(); i = next++) {
        const int M = Ms[i];
        for (int N : Ns)
          for (int K : Ks)
            for (int n_cu : CUs) {
              check_functions(t, M, N, K, n_cu);
              for (int epi = 0; epi < 8; ++epi)
                for (int f16 = 0; f16 < 2; ++f16)
                  for (int variant = 0; variant <= GEMM_V_MAX; ++variant)
                    for (int row0 : {0, 256})
                      for (int stats = 0; stats < 2; ++stats)
                        for (size_t ws : WSs) check_case(t, M, N, K, epi, f16, variant, n_cu, row0, stats != 0, ws);
            }
      }
    });
  for (auto& th : pool) th.join();
  Tally t;
  for (const Tally& x : tallies) t.cases += x.cases, t.failures += x.failures, t.valid += x.valid, t.strips_over_bulk += x.strips_over_bulk;
  printf("gemm plan: %ld cases (%ld valid), %ld failures\n", t.cases, t.valid, t.failures);
  printf("gemm plan: %ld swept shapes have more tail strips than workgroups that own a bulk tile\n", t.strips_over_bulk);
  if (t.failures) return 1;
  printf("gemm plan ok\n");
  return 0;
}
