// ragged_plan_check.cpp -- drives csrc/clipx_ragged_plan.h (the pseudo-samples that pad a ragged text batch to whole GEMM tiles,
// the slot capacities, the CLIP pooling rule) on the CPU.  Its own main, only that header: built with
// -fsanitize=address,undefined by tests/test_ragged_plan_cpu.py and run as a child process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I clip-retrieval_amd/csrc tools/ragged_plan_check.cpp -o ragged_plan_check
// Every slot is a heap block of exactly ragged_slot_ints(B, T, with_rowmap) ints, so a write past the capacity the handles
// allocate is an AddressSanitizer report.  Besides the properties of a plan, every case demands the arrays of the two loops the
// planner replaced (the CLIP text tower's ragged_prepare and the multilingual tower's bert_chunk), restated below as they were.
// Prints nothing unless a check fails, then one summary line and "ragged plan ok"; a failed check prints FAILED, exit status 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "clipx_ragged_plan.h"

using namespace clipx;

static int failures = 0;
static long cases = 0;
#define CHECK(cond)                                                                                                   \
  do {                                                                                                                \
    if (!(cond)) {                                                                                                    \
      if (failures < 40) printf("FAILED %s:%d: %s (B %d T %d pad %d pattern %d)\n", __FILE__, __LINE__, #cond, B, T, P, pattern); \
      ++failures;                                                                                                     \
    }                                                                                                                 \
  } while (0)

struct OldPlan {
  int S;
  std::vector<int> pool, lens, offs, rowmap, src;
};

// ragged_prepare of the CLIP text tower as it was, from behind its length scan (which left lens[0 .. B), pool, longest and M)
static OldPlan old_clip(const std::vector<int>& real, int T, int Mp) {
  const int B = (int)real.size();
  std::vector<int> host((size_t)B * (T + 3) + 3 * 255);  // rg_ints of create_impl
  int* pool = host.data(), *lens = host.data() + B;
  int M = 0, longest = 0;
  for (int b = 0; b < B; ++b) {
    const int len = real[b], best = len - 1;
    lens[b] = len;
    pool[b] = M + best;
    if (len > lens[longest]) longest = b;
    M += len;
  }
  const int lmax = lens[longest];
  const int S = B + (Mp - M + lmax - 1) / lmax;
  for (int b = B, left = Mp - M; b < S; ++b, left -= lmax) lens[b] = std::min(lmax, left);
  int* offs = lens + S, *rowmap = offs + S;
  for (int b = 0, m = 0; b < S; ++b) {
    const int src = b < B ? b : longest;
    offs[b] = m;
    for (int t = 0; t < lens[b]; ++t) rowmap[m + t] = src * T + t;
    m += lens[b];
  }
  OldPlan o;
  o.S = S;
  o.pool.assign(pool, pool + B);
  o.lens.assign(lens, lens + S);
  o.offs.assign(offs, offs + S);
  o.rowmap.assign(rowmap, rowmap + Mp);
  return o;
}

// the top of bert_chunk as it was
static OldPlan old_bert(const std::vector<int>& lens_host, int Mp) {
  const int nb = (int)lens_host.size();
  std::vector<int> host(3 * ((size_t)nb + 255));  // 3 * max_samples of bert_create_impl
  int M = 0, longest = 0;
  for (int b = 0; b < nb; ++b) {
    if (lens_host[b] > lens_host[longest]) longest = b;
    M += lens_host[b];
  }
  const int lmax = lens_host[longest];
  const int S = nb + (Mp - M + lmax - 1) / lmax;
  int *src = host.data(), *lens = host.data() + S, *offs = host.data() + 2 * S;
  for (int b = 0, m = 0, left = Mp - M; b < S; ++b) {
    src[b] = b < nb ? b : longest;
    lens[b] = b < nb ? lens_host[b] : std::min(lmax, left);
    if (b >= nb) left -= lens[b];
    offs[b] = m;
    m += lens[b];
  }
  OldPlan o;
  o.S = S;
  o.src.assign(src, src + S);
  o.lens.assign(lens, lens + S);
  o.offs.assign(offs, offs + S);
  return o;
}

static unsigned rng_state = 12345u;
static int rnd(int lo, int hi) {  // lo .. hi
  rng_state = rng_state * 1664525u + 1013904223u;
  return lo + (int)((rng_state >> 8) % (unsigned)(hi - lo + 1));
}

// pattern 0: all 1, 1: all T, 2: one long among ones (not the first sample where there is a choice), 3: seeded random
static std::vector<int> lengths(int B, int T, int pattern) {
  std::vector<int> v(B, pattern == 1 ? T : 1);
  if (pattern == 2) v[B / 2] = T;
  if (pattern == 3)
    for (int& x : v) x = rnd(1, T);
  return v;
}

static void check_case(const std::vector<int>& real, int T, int P, int pattern) {
  const int B = (int)real.size();
  ++cases;
  int M = 0, first_max = 0;
  for (int b = 0; b < B; ++b) {
    M += real[b];
    if (real[b] > real[first_max]) first_max = b;
  }
  const int Mp = M + P, lmax = real[first_max];
  for (int with_rowmap = 0; with_rowmap < 2; ++with_rowmap) {
    const size_t cap = ragged_slot_ints(B, T, with_rowmap != 0);
    int* slot = (int*)malloc(cap * sizeof(int));
    const int* in = real.data();
    if (with_rowmap) {  // the CLIP tower's call: the lengths already stand in the slot
      memcpy(slot, real.data(), B * sizeof(int));
      in = slot;
    }
    const RaggedPlan p = ragged_complete(slot, in, B, T, Mp, with_rowmap != 0);
    const int S = p.S;
    CHECK(S == B + (P + lmax - 1) / lmax && S <= B + P);
    CHECK((size_t)S <= ragged_max_samples(B) && (size_t)Mp <= ragged_max_rows(B, T));
    CHECK(p.M == M && p.lmax == lmax && p.ints <= cap);
    CHECK(p.ints == 3 * (size_t)S + (with_rowmap ? (size_t)B + Mp : 0));
    if (S >= B) {
      long sum = 0;
      for (int b = 0; b < S; ++b) {
        CHECK(p.offs[b] == sum);
        sum += p.lens[b];
        CHECK(p.src[b] == (b < B ? b : first_max));
        if (b < B) CHECK(p.lens[b] == real[b]);
        else CHECK(p.lens[b] >= 1 && p.lens[b] <= lmax && (p.lens[b] == lmax || b == S - 1));
      }
      CHECK(sum == Mp);
      if (with_rowmap) {
        for (int b = 0; b < S; ++b)
          for (int t = 0; t < p.lens[b]; ++t) CHECK(p.rowmap[p.offs[b] + t] == p.src[b] * T + t);
        for (int b = 0; b < B; ++b) CHECK(p.pool[b] == p.offs[b] + p.lens[b] - 1);
        const OldPlan o = old_clip(real, T, Mp);
        CHECK(o.S == S && std::equal(o.lens.begin(), o.lens.end(), p.lens) && std::equal(o.offs.begin(), o.offs.end(), p.offs));
        CHECK(std::equal(o.pool.begin(), o.pool.end(), p.pool) && std::equal(o.rowmap.begin(), o.rowmap.end(), p.rowmap));
      } else {
        const OldPlan o = old_bert(real, Mp);
        CHECK(o.S == S && std::equal(o.lens.begin(), o.lens.end(), p.lens) && std::equal(o.offs.begin(), o.offs.end(), p.offs));
        CHECK(std::equal(o.src.begin(), o.src.end(), p.src));
      }
    }
    free(slot);
  }
}

static void check_pooling_rule() {
  const int B = 0, P = 0, pattern = -1;
  for (int T : {1, 2, 77, 128}) {
    std::vector<int32_t> row(T, 0);
    CHECK(ragged_pooled_len(row.data(), T) == 1);  // all equal: the first
    for (int at = 0; at < T; ++at) {
      std::fill(row.begin(), row.end(), 7);
      row[at] = 49407;
      CHECK(ragged_pooled_len(row.data(), T) == at + 1);
      for (int again = at + 1; again < T; again += 13) {  // the same maximum later on: still the first
        row[again] = 49407;
        CHECK(ragged_pooled_len(row.data(), T) == at + 1);
      }
      if (at > 0) {  // a smaller id in front, negative ids around
        row[0] = -5;
        row[at - 1] = 49406;
        CHECK(ragged_pooled_len(row.data(), T) == at + 1);
      }
    }
  }
}

static void check_refusals() {
  const int B = 3, T = 77, pattern = -2;
  const int real[3] = {5, 9, 9};
  int slot[16];
  for (int P : {-1, 256, 1000}) {
    for (int& v : slot) v = -77;
    const RaggedPlan p = ragged_complete(slot, real, B, T, 23 + P, true);
    CHECK(p.S == 0 && p.ints == 0);
    for (int v : slot) CHECK(v == -77);  // nothing written
  }
}

int main() {
  for (int T : {1, 2, 77, 128})
    for (int B = 1; B <= 40; ++B)
      for (int pattern = 0; pattern < 4; ++pattern) {
        const std::vector<int> real = lengths(B, T, pattern);
        for (int P = 0; P <= 255; ++P) check_case(real, T, P, pattern);
      }
  // the largest batch a handle is created for by default, at the two ends: the most pseudo-samples (one row each) and the most rows
  for (int T : {128, 1})
    for (int pattern = 0; pattern < 4; ++pattern) check_case(lengths(256, T, pattern), T, 255, pattern);
  check_pooling_rule();
  check_refusals();
  printf("ragged plan: %ld cases, %d failures\n", cases, failures);
  if (failures) return 1;
  printf("ragged plan ok\n");
  return 0;
}
