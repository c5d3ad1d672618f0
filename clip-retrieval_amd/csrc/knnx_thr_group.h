// knnx_thr_group.h -- what a large-k search does BETWEEN two threshold scans of a group of queries (knnx_range.hip:
// search_large_k_thr_locked), and the small host pieces every large-k / range path shares.  No HIP in here: the device is whoever
// answers "how many rows of query i score above thr[i], and which", so that a host-only program can play it
// (tools/thr_group_check.cpp).
//
// A group of gq queries wants kc rows each.  Every step of the caller's loop is
//     thresholds(thr)                      -> one threshold scan of the whole group: counts[gq] (exact even when a slice overflowed),
//                                             the hits of query i in a slice of `cap` entries
//     absorb(counts, cap)                  -> which queries are final and fit (sel[i] = their count), which need larger slices (grow)
//     fetch the sel[i] hits of every query, packed in query order
//     take(hd, hi)                         -> rank them; those queries are done
//     grow ? enlarge the pool (pool_want)  -> the next scan has room for the query that overflowed
// until left == 0.  A query is in one of three states: descending (knnx_descent.h chooses its next threshold), final (its threshold
// stands, but its hits did not fit their slice yet), fetched (it rides along with thr = +INFINITY and counts nothing).
#pragma once

#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>

#include "knnx_descent.h"

namespace knnx {

typedef std::pair<float, int64_t> Hit;  // (score, id)

// the order of every result list: score descending, ties by ascending id
struct HitBetter {
  bool operator()(const Hit& a, const Hit& b) const { return a.first > b.first || (a.first == b.first && a.second < b.second); }
};

// the best `keep` hits of h, in order.  Only they are sorted: O(hits) selection + keep log keep (a threshold scan hands back
// 1.5 .. 16 x keep hits: 10 ms at keep = 100 000 instead of a full sort)
inline void rank_hits(std::vector<Hit>& h, int64_t keep) {
  if ((int64_t)h.size() > keep) {
    std::nth_element(h.begin(), h.begin() + keep, h.end(), HitBetter());
    h.resize((size_t)keep);
  }
  std::sort(h.begin(), h.end(), HitBetter());
}

// the first k of a ranked list into one query's output row, padded with -FLT_MAX / -1
inline void write_topk(const std::vector<Hit>& h, int k, float* Dq, int64_t* Iq) {
  for (int j = 0; j < k; ++j) {
    Dq[j] = j < (int)h.size() ? h[j].first : -FLT_MAX;
    Iq[j] = j < (int)h.size() ? h[j].second : -1;
  }
}

// the hit pool that gives each of `slices` queries room for mx hits: `pool` doubled until it does (pool, slices > 0)
inline size_t pool_want(size_t pool, size_t slices, size_t mx) {
  size_t want = pool;
  while (want / slices < mx) want <<= 1;
  return want;
}

struct ThrGroup {
  enum State { DESCENDING, FINAL, FETCHED };
  struct Step {
    int64_t nsel = 0;    // hits to fetch: the sum of sel[]
    unsigned grow = 0;   // the largest count of a final query that overflowed its slice (0: none did)
    int query_scans = 0; // queries that took part in the scan (not yet fetched when it ran)
  };

  int gq = 0, left = 0;  // queries of the group; those not fetched yet
  int64_t kc = 0;
  std::vector<PqDescent> ds;
  std::vector<State> state;
  std::vector<unsigned> sel;           // the last absorb's selection: count of a query fetched in this step, 0 otherwise
  std::vector<char> picked;            // ... and whether the query was selected (a final query with no hits at all is)
  std::vector<std::vector<Hit>> hits;  // of the fetched queries: the best kc, ranked

  // top: the best `ntop` scores of every query, descending (row i at top + i * ntop; the descent reads the middle and the last one);
  // total[i]: rows in the probed lists of query i
  void start(int nq, int64_t want, const float* top, int ntop, const int64_t* total) {
    gq = left = nq;
    kc = want;
    ds.assign((size_t)nq, PqDescent());
    state.assign((size_t)nq, DESCENDING);
    sel.assign((size_t)nq, 0u);
    picked.assign((size_t)nq, 0);
    hits.assign((size_t)nq, std::vector<Hit>());
    for (int i = 0; i < nq; ++i) ds[i].start(top[(size_t)i * ntop + ntop / 2 - 1], top[(size_t)i * ntop + ntop - 1], kc, total[i]);
  }

  // thr [gq] of the next scan
  void thresholds(float* thr) const {
    for (int i = 0; i < gq; ++i) thr[i] = state[i] == FETCHED ? INFINITY : ds[i].thr;
  }

  // counts [gq] of the scan at thresholds(), cap = entries of one query's slice
  Step absorb(const unsigned* counts, unsigned cap) {
    Step s;
    sel.assign((size_t)gq, 0u);
    picked.assign((size_t)gq, 0);
    for (int i = 0; i < gq; ++i) {
      if (state[i] == FETCHED) continue;
      ++s.query_scans;
      if (state[i] == DESCENDING) {
        if (ds[i].next((int64_t)counts[i]) == PqDescent::SCAN) continue;
        state[i] = FINAL;
      }
      if (counts[i] <= cap) {
        picked[i] = 1;
        sel[i] = counts[i];
        s.nsel += counts[i];
      } else {
        s.grow = std::max(s.grow, counts[i]);
      }
    }
    return s;
  }

  // hd / hi: the hits of the selected queries, sel[i] each, packed in query order and in any order inside a query
  void take(const float* hd, const int64_t* hi) {
    size_t at = 0;
    for (int i = 0; i < gq; ++i) {
      if (!picked[i]) continue;
      std::vector<Hit>& h = hits[i];
      h.resize((size_t)sel[i]);
      for (unsigned j = 0; j < sel[i]; ++j) h[j] = Hit(hd[at + j], hi[at + j]);
      at += sel[i];
      rank_hits(h, kc);
      state[i] = FETCHED;
      --left;
    }
  }
};

}  // namespace knnx
