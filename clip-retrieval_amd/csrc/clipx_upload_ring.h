// clipx_upload_ring.h -- how the stages of the image front end (preprocess / jpeg_kernels / jpeg_huff_kernels .hip) hand a table
// built on the host to their kernels: per device a ring of four slots, each a grow-only device buffer with a page-locked twin of the
// same capacity, guarded by the event of the launches that last read it.  A call builds its table, takes a slot, uploads and
// launches, and commits; `mu` is held from take() through commit().  Every stage keeps a ring of its own.
//
// Lifetime: a ring lives as long as the process.  A stage makes its ring once with `new` behind a function-local static pointer and
// never deletes it, so that no owner's destructor runs during static destruction, when the HIP runtime may already be gone.
#pragma once

#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <mutex>

#include "clipx_host.h"

#pragma GCC visibility push(hidden)  // nothing below is part of the library's ABI

namespace clipx {

struct UploadSlot {
  DevGrow dev;
  PinBuf host;      // page-locked: the upload is a true asynchronous copy
  DevGrow scratch;  // device memory the stage's kernels work in, grown by the stage itself (the pixel stage's planes); else empty
  Event ev;
  bool used = false;
};

struct UploadRing {
  struct PerDevice {
    UploadSlot slot[4];
    int next = 0;
  };
  std::mutex mu;
  const size_t floor;  // smallest capacity a slot is given
  PerDevice dev[64];
  explicit UploadRing(size_t floor_) : floor(floor_) {}

  // The next slot of `device` (0 .. 63, made current by the caller), free of its last reader and with room for `bytes`.  A failure
  // leaves the slot's `used` as it was, and after a failed allocation both buffers are empty.
  int take(int device, size_t bytes, UploadSlot** out) {
    PerDevice& d = dev[device];
    UploadSlot* sl = &d.slot[d.next];
    d.next = (d.next + 1) & 3;
    if (sl->used) HIPCHK(hipEventSynchronize(sl->ev));  // the launch that last used this slot has finished
    if (!sl->ev.e) HIPCHK(sl->ev.create(hipEventDisableTiming));
    if (sl->dev.bytes < bytes || sl->host.bytes < bytes) {
      const size_t want = std::max(bytes, floor);
      hipError_t grow = sl->dev.ensure(want);
      if (grow == hipSuccess) grow = sl->host.ensure(want);
      if (grow != hipSuccess) sl->dev.reset(), sl->host.reset();
      HIPCHK(grow);
    }
    *out = sl;
    return 0;
  }
  // the table through the slot's pinned twin into its device buffer
  static int upload(UploadSlot* sl, const void* table, size_t bytes, hipStream_t st) {
    memcpy(sl->host, table, bytes);
    HIPCHK(hipMemcpyAsync(sl->dev, sl->host, bytes, hipMemcpyHostToDevice, st));
    return 0;
  }
  // behind the caller's launches: the event the slot's next taker waits for
  static int commit(UploadSlot* sl, hipStream_t st) {
    HIPCHK(hipEventRecord(sl->ev, st));
    sl->used = true;
    return 0;
  }
};

}  // namespace clipx

#pragma GCC visibility pop
