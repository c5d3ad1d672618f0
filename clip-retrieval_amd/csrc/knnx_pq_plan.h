// knnx_pq_plan.h -- the sizes of the partial-sum buffer of the M = 256 ADC stage (knnx_ivfpq.hip, knn_pq_kernels.hip).  No device code
// in here: plain 64-bit arithmetic on list sizes, so that a host-only program can drive it (tools/pq_plan_check.cpp).
//
// The lower half of the two-half scan stores one fp32 partial sum per probed row.  A query's sums live in a SLAB of S floats, S = the
// sum of the np largest list sizes of the index: an upper bound of the rows any query can probe, known on the host without asking the
// device.  The g queries scored at once need g x S x 4 bytes; when nq x S x 4 exceeds the budget the pass is cut into consecutive
// sub-groups of g = max(1, budget / (S x 4)) queries (a single query whose slab exceeds the budget gets its slab anyway).
// Every quantity is 64-bit: 256 queries x S x 4 passes 2^31 on a 125 M-row index at nprobe 64.
#pragma once

#include <stdint.h>
#include <algorithm>
#include <functional>
#include <vector>

namespace knnx {

// KNNX_PQ_PARTIAL_MAX_BYTES when the environment does not set it.  A guess: nobody has measured where a larger buffer stops paying.
constexpr uint64_t PQ_PARTIAL_DEFAULT_BYTES = (uint64_t)1 << 30;

// S: the sum of the min(np, nlist) largest of size[0 .. nlist)
inline uint64_t pq_plan_slab(const unsigned* size, int64_t nlist, int64_t np) {
  if (!size || nlist <= 0 || np <= 0) return 0;
  const int64_t take = std::min(np, nlist);
  std::vector<unsigned> v(size, size + nlist);
  if (take < nlist) std::nth_element(v.begin(), v.begin() + take, v.end(), std::greater<unsigned>());
  uint64_t s = 0;
  for (int64_t i = 0; i < take; ++i) s += v[(size_t)i];
  return s;
}

struct PqPlan {
  uint64_t slab = 0;  // S, floats per query
  int nq = 0;         // queries of the pass
  int g = 0;          // queries per sub-group (the last one may hold fewer)

  PqPlan() {}
  PqPlan(uint64_t S, int nq_, uint64_t budget_bytes) : slab(S), nq(std::max(nq_, 0)) {
    const uint64_t per = S * 4;  // bytes of one slab (S < 2^62: it counts rows of an index)
    uint64_t fit = per ? budget_bytes / per : (uint64_t)nq;
    if (fit < 1) fit = 1;
    g = (int)std::min<uint64_t>(fit, (uint64_t)std::max(nq, 1));
  }
  int groups() const { return nq > 0 ? (nq + g - 1) / g : 0; }
  int first(int i) const { return i * g; }                     // first query of sub-group i
  int count(int i) const { return std::min(g, nq - i * g); }   // its queries
  uint64_t base(int q_in_group) const { return (uint64_t)q_in_group * slab; }  // float offset of a query's slab in the buffer
  uint64_t floats() const { return (uint64_t)g * slab; }       // floats the buffer holds
  uint64_t bytes() const { return floats() * 4; }
};

}  // namespace knnx
