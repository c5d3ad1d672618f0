// attn_wide_plan_check.cpp -- drives csrc/clipx_attn_plan.h on the CPU for the head dimensions 88 and 104 (ViT-g/14, ViT-bigG/14 image
// towers).  Its own main, only that header: built with -fsanitize=address,undefined by tests/test_wide_heads_cpu.py and run as a
// child process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I clip-retrieval_amd/csrc tools/attn_wide_plan_check.cpp -o attn_wide_plan_check
// For every T in 1 .. 700 x causal in {0, 1}:
//   dh 88 / 104: a kernel exactly at 1, 2, 3 and 9 key blocks and not causal (attention_kernel, NW = nkb, QPW 1; nine blocks: RECOMP),
//                lds_bytes equal to the one expression of the header restated here and at most ATTN_LDS_LIMIT, every query block owned
//                by one wave for the full and for the pooled launch; ATTN_NONE in every other cell;
//   dh 64 / 80:  every cell what it was before the wide heads came (the table below, restated from the dispatch of that commit).
// Prints one summary line per (dh, causal) and "wide plan ok"; a failed check prints FAILED and the exit status is 1.
#include <stdio.h>

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

// K row bytes, written out: 2 ceil(dh / 16) chunks of 16 B made an odd count; dh 64 is the swizzled 128-B row
static size_t krow_restated(int dh) {
  switch (dh) {
    case 64: return 128;
    case 80: return 176;   // 11 chunks
    case 88: return 208;   // 12 -> 13 chunks
    case 104: return 240;  // 14 -> 15 chunks
    default: return 0;
  }
}
static size_t dv_restated(int dh) { return dh == 64 ? 64 : (dh == 104 ? 128 : 96); }

// The plan of dh 64 / 80 as it was before this program existed: kernel, key blocks, waves, query blocks per wave, RECOMP, LDS bytes
struct Cell { int kernel, nkb, nw, qpw; bool recomp; size_t lds; };
static Cell parent_plan(int T, int dh, int causal) {
  const int nkb = (T + 31) / 32;
  const Cell none{ATTN_NONE, 0, 0, 0, false, 0};
  if (T > 608) return none;
  auto image = [&](int d) { return (size_t)nkb * 32 * (d == 64 ? 128 : 176) + (size_t)(d == 64 ? 64 : 96) * ((size_t)nkb * 64 + 8); };
  if (T > 288) return (dh == 64 && !causal) ? Cell{ATTN_LONG, nkb, 10, 2, false, image(64)} : none;
  if (dh == 80) {
    if (nkb <= 3) return {ATTN_BLOCK, nkb, nkb, 1, false, image(80)};
    if (nkb == 9) return {ATTN_BLOCK, 9, 9, 1, true, image(80)};
    return none;
  }
  switch (nkb) {
    case 1: case 2: case 3: case 4: return {ATTN_BLOCK, nkb, nkb, 1, false, image(64)};
    case 5: case 6: return {ATTN_BLOCK, nkb, 3, 2, false, image(64)};
    case 7: case 8: return {ATTN_BLOCK, nkb, 4, 2, false, image(64)};
    default: return causal ? Cell{ATTN_BLOCK, 9, 3, 3, false, image(64)} : Cell{ATTN_PK9, 9, 6, 2, false, (size_t)2 * (288 * 128 + 2 * 288 * 64)};
  }
}

int main() {
  for (int dh : {88, 104})
    for (int causal : {0, 1}) {
      int n_kernel = 0, n_none = 0;
      size_t max_lds = 0;
      for (int T = 1; T <= 700; ++T) {
        const AttnPlan p = attn_plan(T, dh, causal);
        const int nkb = (T + 31) / 32;
        const bool want = !causal && (nkb <= 3 || nkb == 9);
        if (!want) {
          CHECK(p.kernel == ATTN_NONE && p.lds_bytes == 0 && p.nkb == 0 && p.nw == 0);
          ++n_none;
          continue;
        }
        CHECK(p.kernel == ATTN_BLOCK && p.nkb == nkb && p.nw == nkb && p.qpw == 1 && p.recomp == (nkb == 9));
        const size_t lds = (size_t)nkb * 32 * krow_restated(dh) + dv_restated(dh) * ((size_t)nkb * 64 + 8);
        CHECK(p.lds_bytes == lds && p.lds_bytes == attn_image_bytes(dh, nkb));
        CHECK(attn_krow_bytes(dh) == krow_restated(dh) && attn_dv(dh) == dv_restated(dh));
        CHECK((attn_krow_bytes(dh) / 16) % 2 == 1 && attn_krow_bytes(dh) >= (size_t)2 * ((dh + 15) / 16) * 16);  // odd chunk count, holds every k-step
        CHECK(p.lds_bytes <= ATTN_LDS_LIMIT && p.nw * 64 <= 1024);
        if (p.lds_bytes > max_lds) max_lds = p.lds_bytes;
        for (int q_blocks : {p.nkb, 1}) {
          std::vector<int> owners((size_t)p.nkb, 0);
          for (int w = 0; w < p.nw; ++w)
            for (int qi = 0; qi < p.qpw; ++qi) {
              const int qb = attn_block_of(p, w, qi, q_blocks);
              if (qb < 0) continue;
              CHECK(qb < q_blocks && qb < p.nkb);
              if (qb < p.nkb) ++owners[(size_t)qb];
            }
          for (int qb = 0; qb < p.nkb; ++qb) CHECK(owners[(size_t)qb] == (qb < q_blocks ? 1 : 0));
        }
        ++n_kernel;
      }
      printf("wide dh %d causal %d: %3d planned, %3d refused, largest LDS %zu bytes\n", dh, causal, n_kernel, n_none, max_lds);
    }
  for (int dh : {64, 80})
    for (int causal : {0, 1}) {
      int n_same = 0;
      for (int T = 1; T <= 700; ++T) {
        const AttnPlan p = attn_plan(T, dh, causal);
        const Cell c = parent_plan(T, dh, causal);
        CHECK(p.kernel == c.kernel && p.nkb == c.nkb && p.nw == c.nw && p.qpw == c.qpw && p.recomp == c.recomp && p.lds_bytes == c.lds);
        ++n_same;
      }
      printf("old dh %d causal %d: %3d cells unchanged\n", dh, causal, n_same);
    }
  {
    const int T = 257, dh = 96, causal = 0;
    CHECK(attn_plan(257, 96, 0).kernel == ATTN_NONE && attn_plan(257, 72, 0).kernel == ATTN_NONE && attn_plan(0, 88, 0).kernel == ATTN_NONE);
    CHECK(attn_plan(257, 88, 0).lds_bytes == 115968 && attn_plan(257, 104, 0).lds_bytes == 143872);
  }
  if (failures) {
    printf("%d checks FAILED\n", failures);
    return 1;
  }
  printf("wide plan ok\n");
  return 0;
}
