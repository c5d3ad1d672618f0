// knnx_filter_plan.h -- the integer arithmetic of the device post filter (knnx_search_filtered; include/knnx.h, "Post filter on the
// device").  No device code in here: what the kernels of knn_filter_kernels.hip and the host of knnx_filter.hip share,
// written so that a host-only program can drive every piece against a plain sequential reference (tools/filter_plan_check.cpp).
//
//   * tiles: the k x k similarity matrix of one request is cut into FILTER_TILE x FILTER_TILE tiles and only the tiles (ti, tj) with
//     ti <= tj are visited, one workgroup each.  Tile number t = tj (tj + 1) / 2 + ti (column after column of the upper triangle), so
//     the inverse needs no floating point and does not depend on how many tiles a side has;
//   * scratch: what one request of k results needs on the device (filter_sizes);
//   * components: the rounds of the one-workgroup connected-components kernel, stated sequentially (filter_cc_round, filter_cc).
//     label[x] <= x always names a member of x's component.  A round HOOKS every link whose ends carry different labels -- the larger
//     label's entry takes the smaller label if that is below what it holds -- and then COMPRESSES every label to the root it leads to
//     (label[r] == r).  At the start of a round every label is a root, every value a hook reads or writes is one of those roots, and a
//     hook only ever lowers the entry of such a root below its own index: each round that changes anything therefore retires at least
//     one root, and none comes back.  So at most n - 1 rounds change something, the round after them changes nothing and ends the
//     loop: n rounds are a hard bound, written into the loop.  A quiet round means both ends of every link carry one label, i.e. one
//     root per component, and since label[x] <= x that root is the component's smallest member.  The order in which a round examines
//     its links changes the labels between rounds, never the answer.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace knnx {

constexpr int FILTER_TILE = 64;                    // rows and columns of one tile of the similarity matrix (2 x 2 waves of 32 x 32)
constexpr int FILTER_MAX_K = 8192;                 // = KNNX_FILTER_MAX_K: the labels of the components kernel are k x 4 B of LDS
constexpr int64_t FILTER_LINK_CAP = (int64_t)1 << 20;  // links kept on the device (i << 16 | j, i < j < 8192)

struct FilterTileXY {
  int ti, tj;  // ti <= tj
};

constexpr int filter_tiles_side(int n) { return (n + FILTER_TILE - 1) / FILTER_TILE; }
constexpr int filter_tiles(int nt) { return nt * (nt + 1) / 2; }
constexpr int filter_tile_index(int ti, int tj) { return tj * (tj + 1) / 2 + ti; }
// the inverse: tj = the largest c with c (c + 1) / 2 <= t (bisection in integers; t < 2^29), ti = what is left
constexpr FilterTileXY filter_tile(int t) {
  int lo = 0, hi = 1 << 15;
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (mid * (mid + 1) / 2 <= t) lo = mid;
    else hi = mid;
  }
  return FilterTileXY{t - lo * (lo + 1) / 2, lo};
}

constexpr uint32_t filter_link(int i, int j) { return ((uint32_t)i << 16) | (uint32_t)j; }
constexpr int filter_link_i(uint32_t l) { return (int)(l >> 16); }
constexpr int filter_link_j(uint32_t l) { return (int)(l & 0xffffu); }

// device scratch of one request, in elements of each buffer's type (FilterScratch in knnx_host.h allocates exactly these)
struct FilterSizes {
  size_t rows;      // float   [k][d]          the gathered rows, normalised in place
  size_t ids;       // int64   [k]
  size_t links;     // uint32  [FILTER_LINK_CAP]
  size_t counters;  // int32   [FILTER_COUNTERS]
  size_t vscores;   // float   [k][violence outputs]
  size_t sscores;   // float   [k][safety outputs]
  size_t drop;      // uint8   [k]
  size_t bytes() const { return rows * 4 + ids * 8 + links * 4 + counters * 4 + vscores * 4 + sscores * 4 + drop; }
};
// counters: links found (also past the cap), rounds the components kernel ran, 1 if it reached its bound
enum { FILTER_C_LINKS = 0, FILTER_C_ROUNDS = 1, FILTER_C_BOUND = 2, FILTER_COUNTERS = 4 };

inline FilterSizes filter_sizes(int k, int d, int v_out, int s_out) {
  FilterSizes s;
  s.rows = (size_t)k * (size_t)d;
  s.ids = (size_t)k;
  s.links = (size_t)FILTER_LINK_CAP;
  s.counters = FILTER_COUNTERS;
  s.vscores = (size_t)k * (size_t)std::max(v_out, 1);
  s.sscores = (size_t)k * (size_t)std::max(s_out, 1);
  s.drop = (size_t)k;
  return s;
}

// one round over m links; false: nothing changed (the labels are final)
inline bool filter_cc_round(std::vector<int32_t>& label, const uint32_t* links, int64_t m) {
  bool changed = false;
  for (int64_t e = 0; e < m; ++e) {
    const int32_t a = label[(size_t)filter_link_i(links[e])], b = label[(size_t)filter_link_j(links[e])];
    if (a == b) continue;
    const int32_t hi = std::max(a, b), lo = std::min(a, b);
    label[(size_t)hi] = std::min(label[(size_t)hi], lo);
    changed = true;
  }
  if (!changed) return false;
  for (size_t x = 0; x < label.size(); ++x) {
    int32_t r = label[x];
    while (label[(size_t)r] != r) r = label[(size_t)r];
    label[x] = r;
  }
  return true;
}

// labels of n nodes under m links: 0 and the rounds run (the quiet one included), or 1 when n rounds did not end it (cannot happen:
// see the head of this file; the kernel reports the same condition and the host turns it into KNNX_E_STATE)
inline int filter_cc(int n, const uint32_t* links, int64_t m, std::vector<int32_t>& label, int& rounds) {
  label.resize((size_t)n);
  for (int x = 0; x < n; ++x) label[(size_t)x] = x;
  for (rounds = 0; rounds < n;) {
    ++rounds;
    if (!filter_cc_round(label, links, m)) return 0;
  }
  return n > 0 ? 1 : 0;
}

}  // namespace knnx
