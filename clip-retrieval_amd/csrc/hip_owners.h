// hip_owners.h -- the owners of device memory, pinned memory, streams, events and graph execs that both host layers build their
// handles from (knnx_host.h, clipx_host.h), as do the image front end's upload ring (clipx_upload_ring.h) and postfilter.hip.
// Move-only; each converts to the raw handle it holds, so it is passed to launchers and copies like that handle.  The HIP runtime
// only: no error codes of either ABI, nothing else of the project.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <type_traits>
#include <utility>

#pragma GCC visibility push(hidden)  // nothing below is part of the library's ABI

// One device allocation of n T (bytes for T = void).  Move-only; converts to T* so that it is passed to launchers and
// copies like the pointer it holds.  borrow() points it at memory somebody else owns (attached rows, a device-resident
// training sample): reset() and the destructor then leave that memory alone.
template <class T>
struct DevBuf {
  T* p = nullptr;
  bool borrowed = false;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), borrowed(o.borrowed) { o.p = nullptr, o.borrowed = false; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(p, o.p);
      std::swap(borrowed, o.borrowed);
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  hipError_t alloc(size_t n) {
    reset();
    hipError_t e = hipMalloc((void**)&p, n * sizeof(std::conditional_t<std::is_void<T>::value, char, T>));
    if (e != hipSuccess) p = nullptr;
    return e;
  }
  void borrow(const void* q) {
    reset();
    p = (T*)q;
    borrowed = true;
  }
  void reset() {
    if (p && !borrowed) (void)hipFree(p);
    p = nullptr;
    borrowed = false;
  }
  operator T*() const { return p; }
};
// `e` carries the first failure of a chain of allocations; the ones after it are skipped
template <class T>
inline void dev_alloc(hipError_t& e, DevBuf<T>& b, size_t n) {
  if (e == hipSuccess) e = b.alloc(n);
}

// grow-only pinned staging buffer
struct PinBuf {
  void* p = nullptr;
  size_t bytes = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { reset(); }
  hipError_t ensure(size_t want) {
    if (bytes >= want) return hipSuccess;
    reset();
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) p = nullptr;
    else bytes = want;
    return e;
  }
  void reset() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
  operator void*() const { return p; }
};

// grow-only device buffer of bytes, PinBuf's device twin (a DevBuf keeps no capacity); empty again after a failed ensure()
struct DevGrow {
  DevBuf<void> buf;
  size_t bytes = 0;
  hipError_t ensure(size_t want) {
    if (bytes >= want) return hipSuccess;
    bytes = 0;
    hipError_t e = buf.alloc(want);
    if (e == hipSuccess) bytes = want;
    return e;
  }
  void reset() {
    buf.reset();
    bytes = 0;
  }
  operator void*() const { return buf.p; }
};

struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
  Stream& operator=(Stream&& o) noexcept {
    std::swap(s, o.s);
    return *this;
  }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  operator hipStream_t() const { return s; }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept {
    std::swap(e, o.e);
    return *this;
  }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
  operator hipEvent_t() const { return e; }
};

// an instantiated hipGraph (adopted from hipGraphInstantiate, never created here)
struct GraphExec {
  hipGraphExec_t g = nullptr;
  GraphExec() = default;
  explicit GraphExec(hipGraphExec_t g_) : g(g_) {}
  GraphExec(const GraphExec&) = delete;
  GraphExec& operator=(const GraphExec&) = delete;
  GraphExec(GraphExec&& o) noexcept : g(o.g) { o.g = nullptr; }
  GraphExec& operator=(GraphExec&& o) noexcept {
    std::swap(g, o.g);
    return *this;
  }
  ~GraphExec() {
    if (g) (void)hipGraphExecDestroy(g);
  }
  operator hipGraphExec_t() const { return g; }
};

#pragma GCC visibility pop
