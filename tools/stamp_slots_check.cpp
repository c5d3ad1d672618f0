// stamp_slots_check.cpp -- the bookkeeping of the profiler's stamp slots (csrc/clipx_stamp_slots.h) without a GPU: StampBook,
// stamp_reduce on hand-made slots, and the plans (csrc/clipx_gemm_plan.h) of the shapes the GPU tests reach each launch site with.  Its own main; built with
// -fsanitize=address,undefined and run as a child by tests/test_stamp_slots_cpu.py.
//
//   g++ -std=c++17 -O2 -g -fsanitize=address,undefined -I clip-retrieval_amd/csrc tools/stamp_slots_check.cpp -o stamp_slots_check
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "clipx_gemm_plan.h"
#include "clipx_stamp_slots.h"

using namespace clipx;

static int failures = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      ++failures;                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);         \
    }                                                               \
  } while (0)

// bursts of hand-outs between reads: ids are consecutive from 0, a chunk is needed exactly when the ids run out, runs() covers
// [0, next) once with one run per chunk, reset() frees everything and keeps the chunks
static long long book_cases(int chunk_slots) {
  StampBook b(chunk_slots);
  long long steps = 0;
  CHECK(b.take() == -1 && b.capacity() == 0 && b.runs().empty());
  unsigned r = 12345u + (unsigned)chunk_slots;
  int most = 0;
  for (int round = 0; round < 200; ++round) {
    r = r * 1664525u + 1013904223u;
    const int burst = 1 + (int)((r >> 8) % (unsigned)(3 * chunk_slots + 2));
    for (int i = 0; i < burst; ++i, ++steps) {
      int id = b.take();
      if (id < 0) {
        CHECK(b.in_use() == b.capacity());
        const int before = b.capacity();
        b.add_chunk();
        CHECK(b.capacity() == before + chunk_slots);
        id = b.take();
      }
      CHECK(id == i && b.in_use() == i + 1);
    }
    most = burst > most ? burst : most;
    CHECK(b.capacity() == (most + chunk_slots - 1) / chunk_slots * chunk_slots);  // never more chunks than the largest burst needed
    const auto runs = b.runs();
    int covered = 0;
    for (size_t i = 0; i < runs.size(); ++i) {
      CHECK(runs[i].first == covered && runs[i].first % chunk_slots == 0);
      CHECK(runs[i].second > 0 && runs[i].second <= chunk_slots);
      CHECK(i + 1 == runs.size() || runs[i].second == chunk_slots);
      covered += runs[i].second;
    }
    CHECK(covered == burst);
    b.reset();
    CHECK(b.in_use() == 0 && b.runs().empty());
  }
  return steps;
}

// The shapes tests/test_profile_stamps_gpu.py reaches the launch sites with: each must still plan onto the kernels it is there for.
static void plan_cases() {
  const size_t ws = (size_t)32 << 20;  // the handle's split-K scratch
  const int V = GEMM_V_DEFAULT, CU = 256;
  GemmPlan p = gemm_plan(8192, 1024, 1024, EPI_BIAS_F16, true, V, CU, 0, false, 0);
  CHECK(p.valid && p.kernel256 == GEMM256_W4 && p.rows256 == 8192 && p.rows128 == 0 && p.stats_rows == 0);
  p = gemm_plan(8192, 1024, 640, EPI_TABLE_F32, false, V, CU, 0, false, 0);
  CHECK(p.valid && p.kernel256 == GEMM256_W8 && p.rows256 == 8192 && p.rows128 == 0);
  p = gemm_plan(8224, 1024, 1024, EPI_BIAS_RESID_H16, false, V, CU, 0, false, 0);
  CHECK(p.valid && p.kernel256 == GEMM256_W4 && p.rows256 == 8192 && p.tail_nb == 0 && p.rows128 == 32 && p.splitk == 1);
  p = gemm_plan(300, 768, 768, EPI_BIAS_BF16, false, V, CU, 0, false, 0);
  CHECK(p.valid && p.kernel256 == GEMM256_NONE && p.rows128 == 300 && p.splitk == 1);
  // the B = 1 text query of ViT-B/32 (77 rows of width 512; the pooled last block: 1 row): QKV, out-proj, fc1, fc2
  for (int M : {77, 1}) {
    const int shapes[4][4] = {{1536, 512, EPI_BIAS_F16, 1}, {512, 512, EPI_BIAS_RESID_H16, 0}, {2048, 512, EPI_BIAS_QGELU_BF16, 1}, {512, 2048, EPI_BIAS_RESID_H16, 0}};
    for (auto& sh : shapes) {
      p = gemm_plan(M, sh[0], sh[1], sh[2], sh[3] != 0, V, CU, 0, false, ws);
      CHECK(p.valid && p.kernel256 == GEMM256_NONE && p.rows128 == M && p.splitk > 1);
    }
  }
  p = gemm_plan(300, 768, 768, EPI_BIAS_RESID_H16, true, V, CU, 0, false, 0);  // the refused launch of the tests
  CHECK(!p.valid);
}

static void reduce_cases() {
  StampSlot s;
  unsigned long long a = 0, b = 0;
  for (int i = 0; i < STAMP_WAYS; ++i) s.way[i] = StampEntry{STAMP_FILL_START, STAMP_FILL_END};
  CHECK(!stamp_reduce(s, &a, &b));  // as filled: no kernel stamped it
  s.way[STAMP_WAYS - 1] = StampEntry{100, 250};
  CHECK(stamp_reduce(s, &a, &b) && a == 100 && b == 250);
  s.way[0] = StampEntry{90, STAMP_FILL_END};  // a workgroup that started and (another way) ended
  CHECK(stamp_reduce(s, &a, &b) && a == 90 && b == 250);
  if (STAMP_WAYS > 2) {
    s.way[1] = StampEntry{STAMP_FILL_START, 300};
    CHECK(stamp_reduce(s, &a, &b) && a == 90 && b == 300);
  }
  for (int i = 0; i < STAMP_WAYS; ++i) s.way[i] = StampEntry{500, STAMP_FILL_END};
  CHECK(!stamp_reduce(s, &a, &b));  // started, never ended
  for (int i = 0; i < STAMP_WAYS; ++i) s.way[i] = StampEntry{500, 400};
  CHECK(!stamp_reduce(s, &a, &b));  // an end in front of the start is not a time
  CHECK(sizeof(StampSlot) == (size_t)STAMP_WAYS * 16);
}

int main() {
  long long steps = 0;
  for (int cs : {1, 2, 3, 7, 64, 1000}) steps += book_cases(cs);
  reduce_cases();
  plan_cases();
  printf("stamp slots: %lld hand-outs over 6 chunk sizes, %d failures\n", steps, failures);
  if (failures == 0) printf("stamp slots ok\n");
  return failures ? 1 : 0;
}
