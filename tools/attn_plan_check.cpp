// attn_plan_check.cpp -- drives csrc/clipx_attn_plan.h (which attention kernel runs, with how many key blocks, how much LDS, and
// which wave owns which query block) on the CPU.  Its own main, only that header: built with -fsanitize=address,undefined by
// tests/test_long_seq_cpu.py and run as a child process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I clip-retrieval_amd/csrc tools/attn_plan_check.cpp -o attn_plan_check
// For every T in 1 .. 700 x dh in {64, 80} x causal in {0, 1} it prints nothing unless a check fails, then one summary line per
// (dh, causal) and "attn plan ok"; a failed check prints FAILED and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "clipx_attn_plan.h"

using namespace clipx;

static int failures = 0;
#define CHECK(cond)                                                                                          \
  do {                                                                                                       \
    if (!(cond)) {                                                                                           \
      if (failures < 40) printf("FAILED %s:%d: %s (T %d dh %d causal %d)\n", __FILE__, __LINE__, #cond, T, dh, causal); \
      ++failures;                                                                                            \
    }                                                                                                        \
  } while (0)

// The dispatch of launch_attention as it was before the long-sequence kernel, restated from its switch statements: the kernel, the
// waves and the query blocks per wave of every T <= 288 (kernel 0: hipErrorInvalidValue).
struct Old { int kernel, nw, qpw; bool recomp; };
static Old old_dispatch(int T, int dh, int causal) {
  const int nkb = (T + 31) / 32;
  if (dh == 80) {
    switch (nkb) {
      case 1: return {ATTN_BLOCK, 1, 1, false};
      case 2: return {ATTN_BLOCK, 2, 1, false};
      case 3: return {ATTN_BLOCK, 3, 1, false};
      case 9: return {ATTN_BLOCK, 9, 1, true};
      default: return {ATTN_NONE, 0, 0, false};
    }
  }
  switch (nkb) {
    case 1: return {ATTN_BLOCK, 1, 1, false};
    case 2: return {ATTN_BLOCK, 2, 1, false};
    case 3: return {ATTN_BLOCK, 3, 1, false};
    case 4: return {ATTN_BLOCK, 4, 1, false};
    case 5: return {ATTN_BLOCK, 3, 2, false};
    case 6: return {ATTN_BLOCK, 3, 2, false};
    case 7: return {ATTN_BLOCK, 4, 2, false};
    case 8: return {ATTN_BLOCK, 4, 2, false};
    case 9: return causal ? Old{ATTN_BLOCK, 3, 3, false} : Old{ATTN_PK9, 6, 2, false};
    default: return {ATTN_NONE, 0, 0, false};
  }
}

int main() {
  for (int dh : {64, 80})
    for (int causal : {0, 1}) {
      int n_old = 0, n_long = 0, n_none = 0;
      size_t max_lds = 0;
      for (int T = 1; T <= 700; ++T) {
        const AttnPlan p = attn_plan(T, dh, causal);
        const int nkb = (T + 31) / 32;
        if (T <= 288) {
          const Old o = old_dispatch(T, dh, causal);
          CHECK(p.kernel == o.kernel);
          CHECK(p.kernel != ATTN_LONG);
          if (o.kernel != ATTN_NONE) {
            CHECK(p.nkb == nkb && p.nw == o.nw && p.qpw == o.qpw && p.recomp == o.recomp);
            // the bytes launch_attention_cfg / launch_attention_pk9 have always asked for
            const size_t krow = dh == 64 ? 128 : 176, dv = dh == 64 ? 64 : 96;
            CHECK(krow == attn_krow_bytes(dh) && dv == attn_dv(dh));  // the one expression every launcher takes them from
            const size_t want = o.kernel == ATTN_PK9 ? (size_t)2 * (288 * 128 + 2 * 288 * 64) : (size_t)nkb * 32 * krow + dv * ((size_t)nkb * 64 + 8);
            CHECK(p.lds_bytes == want);
            ++n_old;
          } else {
            ++n_none;
          }
        } else if (T <= 608 && dh == 64 && !causal) {
          CHECK(p.kernel == ATTN_LONG);
          CHECK(p.nkb == nkb && p.nkb >= 10 && p.nkb <= 19);
          CHECK(p.nw == ATTN_LONG_NW && p.qpw == ATTN_LONG_QPW && p.nw * p.qpw >= p.nkb);
          CHECK(p.lds_bytes == (size_t)nkb * 32 * 128 + (size_t)64 * (nkb * 64 + 8));
          ++n_long;
        } else {
          CHECK(p.kernel == ATTN_NONE);
          ++n_none;
        }
        if (p.kernel == ATTN_NONE) {
          CHECK(p.lds_bytes == 0 && p.nkb == 0);
          continue;
        }
        CHECK(p.lds_bytes <= ATTN_LDS_LIMIT && p.lds_bytes <= 163840);
        CHECK(p.nw * 64 <= 1024);
        if (p.lds_bytes > max_lds) max_lds = p.lds_bytes;
        if (p.kernel == ATTN_PK9) continue;  // the persistent kernel deals its nine blocks by a role table of its own
        // every query block below q_blocks is owned by exactly one (wave, slot), for the full launch and for the pooled one
        for (int q_blocks : {p.nkb, 1}) {
          std::vector<int> owners((size_t)p.nkb, 0);
          for (int w = 0; w < p.nw; ++w)
            for (int qi = 0; qi < p.qpw; ++qi) {
              const int qb = attn_block_of(p, w, qi, q_blocks);
              if (qb < 0) continue;
              CHECK(qb < q_blocks && qb < p.nkb);
              if (qb >= 0 && qb < p.nkb) ++owners[(size_t)qb];
              CHECK(attn_wave_of(p, qb) == w && attn_slot_of(p, qb) == qi);
            }
          for (int qb = 0; qb < p.nkb; ++qb) CHECK(owners[(size_t)qb] == (qb < q_blocks ? 1 : 0));
        }
      }
      printf("plan dh %d causal %d: %3d old, %3d long, %3d refused, largest LDS %zu bytes\n", dh, causal, n_old, n_long, n_none, max_lds);
    }
  // out-of-range arguments are refused, not planned
  {
    const int T = 0, dh = 64, causal = 0;
    CHECK(attn_plan(0, 64, 0).kernel == ATTN_NONE && attn_plan(-5, 64, 0).kernel == ATTN_NONE);
    CHECK(attn_plan(257, 72, 0).kernel == ATTN_NONE && attn_plan(257, 96, 0).kernel == ATTN_NONE);  // (88 and 104: tools/attn_wide_plan_check.cpp)
    CHECK(attn_plan(577, 64, 0).nkb == 19 && attn_plan(577, 64, 0).lds_bytes == 156160);
  }
  if (failures) {
    printf("%d checks FAILED\n", failures);
    return 1;
  }
  printf("attn plan ok\n");
  return 0;
}
