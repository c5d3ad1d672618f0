// clipx_stamp_slots.h -- the slots the GEMM kernels write their own start and end times into (the GEMM brackets of
// clipx_profile_enable), and the bookkeeping of the pool they are handed out from.  System includes only: the
// bookkeeping is checked on the CPU (tools/stamp_slots_check.cpp); the device memory behind it belongs to clipx_host.h's Profiler.
//
// A slot belongs to ONE kernel launch.  It is STAMP_WAYS entries of {first_start, last_end} in ticks of the constant-rate counter
// (wall_clock64(), hipDeviceAttributeWallClockRate): workgroup b does atomicMin / atomicMax on entry b % STAMP_WAYS, the host takes
// the minimum / maximum over the entries.  One entry for all workgroups would put a launch's 256 end stamps on one address in the
// same microsecond (a persistent GEMM's workgroups finish together) and the memory side serialises same-address atomics; 64 entries
// leave four workgroups per address.  A slot is handed out FILLED ({~0, 0} in every entry) and refilled when it has been read.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>

namespace clipx {

#ifndef CLIPX_STAMP_WAYS
#define CLIPX_STAMP_WAYS 64
#endif
constexpr int STAMP_WAYS = CLIPX_STAMP_WAYS;  // a power of two
static_assert(STAMP_WAYS > 0 && (STAMP_WAYS & (STAMP_WAYS - 1)) == 0, "STAMP_WAYS: a power of two");

struct StampEntry {
  unsigned long long first_start, last_end;
};
struct StampSlot {
  StampEntry way[STAMP_WAYS];
};
constexpr unsigned long long STAMP_FILL_START = ~0ull, STAMP_FILL_END = 0ull;

// first start / last end of one slot as read back; false: some kernel that was given the slot never stamped it
inline bool stamp_reduce(const StampSlot& s, unsigned long long* start, unsigned long long* end) {
  unsigned long long a = STAMP_FILL_START, b = STAMP_FILL_END;
  for (int i = 0; i < STAMP_WAYS; ++i) {
    a = std::min(a, s.way[i].first_start);
    b = std::max(b, s.way[i].last_end);
  }
  *start = a;
  *end = b;
  return a != STAMP_FILL_START && b != STAMP_FILL_END && a <= b;
}

// Which slots are free.  Slot ids count through the chunks: id = chunk * chunk_slots + index.  Every stamp scope is a GEMM scope and
// clipx_profile_get reads all of them together, so the book is a bump counter: take() hands out the next id, reset() (the read)
// starts again at 0, runs() lists what was handed out as one run per chunk (what is copied back and refilled).
struct StampBook {
  int chunk_slots;
  int chunks = 0;
  int next = 0;  // ids [0, next) are handed out
  explicit StampBook(int chunk_slots_) : chunk_slots(chunk_slots_) {}
  int capacity() const { return chunks * chunk_slots; }
  int in_use() const { return next; }
  void add_chunk() { ++chunks; }  // (its device memory exists and is filled)
  int take() { return next < capacity() ? next++ : -1; }  // -1: none free (the caller adds a chunk)
  void reset() { next = 0; }
  // [first, first + count) per chunk that has ids handed out
  std::vector<std::pair<int, int>> runs() const {
    std::vector<std::pair<int, int>> r;
    for (int first = 0; first < next; first += chunk_slots) r.emplace_back(first, std::min(chunk_slots, next - first));
    return r;
  }
};

}  // namespace clipx
