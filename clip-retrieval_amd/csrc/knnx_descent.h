// knnx_descent.h -- the per-query threshold descent of a large-k search on an IVF-PQ or IVF-SQ8 index (knnx_thr_group.h runs one per
// query of a group).  No HIP in here: a struct and next(count) -> {threshold | fetch}, so that a host-only program can drive it
// (tools/descent_check.cpp).
//
// A threshold scan returns every row of the probed lists whose score is > thr (strict) and counts them exactly.  The descent looks
// for a threshold that lets at least `want` rows through and not absurdly many more, with the rule search_large_k_locked uses for
// IVF indexes (knnx_range.hip):
//   * first step from the LOCAL score density: 32 rows lie between the 32nd and the 64th best score, so k - 64 more rows are about
//     (k - 64) / 32 such gaps below the 64th (fewer: the density grows away from the top);
//   * while count < want the step doubles;
//   * a step that overshoots (count > 16 want and > 65 536) is bisected back towards the last threshold that had too few, at most
//     4 times;
//   * three ever lower thresholds with the same count: the probed lists hold no more rows -- take everything (thr = -FLT_MAX).
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>

namespace knnx {

struct PqDescent {
  enum Action { SCAN, FETCH };
  static constexpr int MAX_BISECT = 4;
  static constexpr int MAX_STEPS = 60;           // doublings before the descent gives up and takes everything
  static constexpr int64_t OVERSHOOT_MIN = 65536;

  int64_t want = 0;        // min(kc, rows in the probed lists) is what the caller needs; the descent is told kc
  float thr = -FLT_MAX;    // threshold of the scan to run next / of the scan whose hits are fetched
  float thr_hi = FLT_MAX;  // lowest threshold known to let fewer than `want` rows through
  float lo_ok = -FLT_MAX;  // a threshold known to let >= want rows through (bisection bracket)
  float step = 0.f;
  int64_t prev_cnt = -1;
  int stalled = 0, bisections = 0, it = 0;
  int scans = 0;           // threshold scans asked for so far

  // s32 / s64: the 32nd and 64th best score of the query; kc: rows wanted; total: rows in the query's probed lists
  void start(float s32, float s64, int64_t kc, int64_t total) {
    *this = PqDescent();
    want = std::min<int64_t>(kc, total);
    if (total <= 2 * kc) {  // everything in one scan, no descent
      thr = -FLT_MAX;
    } else {
      step = std::max((s32 - s64) * std::min(64.f, (float)(kc - 64) / 32.f) * 0.5f, 1e-4f * std::max(1.f, fabsf(s64)));
      thr = s64 - step;
      if (!(thr > -FLT_MAX)) thr = -FLT_MAX;  // (also a NaN)
      thr_hi = s64;
    }
    scans = 1;
  }

  // the scan at `thr` counted cnt rows: SCAN -> run another at the new thr; FETCH -> the hits of this scan are the answer
  Action next(int64_t cnt) {
    stalled = (cnt == prev_cnt) ? stalled + 1 : 0;
    prev_cnt = cnt;
    if (cnt < want && thr > -FLT_MAX && stalled < 3 && it < MAX_STEPS) {
      ++it;
      thr_hi = thr;
      step *= 2.f;
      thr = (thr - step > -FLT_MAX) ? thr - step : -FLT_MAX;
      if (lo_ok > -FLT_MAX && !(thr > lo_ok)) thr = lo_ok;  // below a threshold known to be enough there is nothing to learn
      ++scans;
      return SCAN;
    }
    if (cnt < want && thr > -FLT_MAX) {  // stalled or out of patience: everything the scan can reach
      thr = -FLT_MAX;
      stalled = 0;
      ++scans;
      return SCAN;
    }
    if (cnt > 16 * want && cnt > OVERSHOOT_MIN && bisections < MAX_BISECT && thr_hi < FLT_MAX && thr > -FLT_MAX) {
      const float mid = 0.5f * (thr + thr_hi);
      if (mid > thr && mid < thr_hi) {  // (two neighbouring floats cannot be bisected)
        lo_ok = thr;
        thr = mid;
        ++bisections;
        step = 0.5f * (thr - lo_ok);  // a middle that has too few rows steps down again, towards lo_ok
        ++scans;
        return SCAN;
      }
    }
    return FETCH;
  }
};

}  // namespace knnx
