// clipx_host_path.hip -- the entry points of include/clipx.h that take HOST buffers: the synchronous calls and the tickets.
//
// A chunk (<= host_chunk samples) travels through one staging slot: upload on the copy stream (straight
// from caller memory when that is already page-locked -- the reference's DataLoader collates with pin_memory, reader.py:198
// -- otherwise through the slot's pinned buffer), kernels + download on the compute stream, copy-out to the caller when
// the slot is collected.  The upload of a later chunk runs while the kernels of an earlier one execute; the activation
// workspace is shared, so the compute stream serialises the chunks.  Chunking never changes a row's result (test: bitwise).

#include "clipx_host.h"

using namespace clipx;

struct clipx_ticket {
  clipx_handle* h;
  int slot;
  int nb;
  uint16_t* out16;
  float* out32;
};

// caller holds h->mu.  Returns the slot index (>= 0) or a negative error code.
static int slot_submit(clipx_handle* h, int kind, bool single_query, const char* src, size_t in_bytes_per_item, int nb, int pix_fmt, bool want32) {
  StagingSlots& S = h->slots;
  int s = -1;
  for (int i = 0; i < StagingSlots::N; ++i) {
    const int c = (S.next + i) % StagingSlots::N;
    if (!S.busy[c]) { s = c; break; }
  }
  if (s < 0) return fail(CLIPX_E_STATE, "all staging slots are in flight: clipx_wait() an earlier ticket first");
  S.next = (s + 1) % StagingSlots::N;
  hipPointerAttribute_t attr;
  bool pinned = false;
  if (hipPointerGetAttributes(&attr, src) == hipSuccess) pinned = attr.type == hipMemoryTypeHost;
  else (void)hipGetLastError();  // plain malloc memory: the query fails, which is the answer
  if (!pinned) {
    memcpy(S.pin_in[s], src, (size_t)nb * in_bytes_per_item);
    src = (const char*)S.pin_in[s].p;
  }
  const size_t E = h->desc.embed_dim;
  hipStream_t st = h->stream;
  HIPCHK(hipMemcpyAsync(S.dev_in[s], src, (size_t)nb * in_bytes_per_item, hipMemcpyHostToDevice, h->copy_stream));
  HIPCHK(hipEventRecord(S.copied[s], h->copy_stream));
  HIPCHK(hipStreamWaitEvent(st, S.copied[s], 0));
  int r = h->gate.acquire(st);
  if (r) return r;
  float* o32 = want32 ? S.dev_out32[s].p : nullptr;
  // (text: the ragged tower reads the ids on the host, from where the upload took them)
  const Call c{st, single_query, h->range.flag(s), kind == KIND_TEXT ? reinterpret_cast<const int32_t*>(src) : nullptr};
  r = kind == KIND_IMAGE ? vision_chunk(h, c, S.dev_in[s], nb, pix_fmt, S.dev_out[s], o32)
                         : text_chunk(h, c, (const int32_t*)S.dev_in[s].p, nb, S.dev_out[s], o32);
  if (r) return r;
  if ((r = h->gate.release(st))) return r;
  char* po = (char*)S.pin_out[s].p;
  HIPCHK(hipMemcpyAsync(po, S.dev_out[s], (size_t)nb * E * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  if (want32) HIPCHK(hipMemcpyAsync(po + S.out_bytes, o32, (size_t)nb * E * sizeof(float), hipMemcpyDeviceToHost, st));
  if ((r = h->range.read_back(s, st))) return r;
  HIPCHK(hipEventRecord(S.done[s], st));
  S.busy[s] = true;
  return s;
}

// blocks until the slot's chunk is complete, copies it out, frees the slot.  Caller holds h->mu or owns the ticket.
static int slot_collect(clipx_handle* h, int s, int nb, uint16_t* out16, float* out32) {
  StagingSlots& S = h->slots;
  const size_t E = h->desc.embed_dim;
  hipError_t e = hipEventSynchronize(S.done[s]);
  if (e == hipSuccess) {
    const char* po = (const char*)S.pin_out[s].p;
    if (out16) memcpy(out16, po, (size_t)nb * E * sizeof(uint16_t));
    if (out32) memcpy(out32, po + S.out_bytes, (size_t)nb * E * sizeof(float));
  }
  S.busy[s] = false;
  if (e != hipSuccess) return fail(CLIPX_E_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(e));
  return h->range.test_and_clear(s) ? RangeGuard::overflow() : 0;
}

// synchronous call: chunks pipelined two deep through the slots
static int host_sync(clipx_handle* h, int kind, const char* in, size_t in_bytes_per_item, int B, int pix_fmt, uint16_t* out16,
                     float* out32) {
  const size_t E = h->desc.embed_dim;
  const int CH = h->host_chunk;
  const int nchunk = (B + CH - 1) / CH;
  int prev_slot = -1, prev_o = 0, prev_nb = 0;
  for (int c = 0; c < nchunk; ++c) {
    const int o = c * CH, nb = std::min(CH, B - o);
    const int s = slot_submit(h, kind, B == 1, in + (size_t)o * in_bytes_per_item, in_bytes_per_item, nb, pix_fmt, out32 != nullptr);
    if (s < 0) return s;
    if (prev_slot >= 0) {
      int r = slot_collect(h, prev_slot, prev_nb, out16 ? out16 + (size_t)prev_o * E : nullptr, out32 ? out32 + (size_t)prev_o * E : nullptr);
      if (r) return r;
    }
    prev_slot = s; prev_o = o; prev_nb = nb;
  }
  if (prev_slot >= 0)
    return slot_collect(h, prev_slot, prev_nb, out16 ? out16 + (size_t)prev_o * E : nullptr, out32 ? out32 + (size_t)prev_o * E : nullptr);
  return 0;
}

static int encode_image_host(clipx_handle* h, const void* pixels, int B, int pix_fmt, uint16_t* out16, float* out32) {
  if (!h || (B > 0 && (!pixels || (!out16 && !out32))) || B < 0) return fail(CLIPX_E_ARG, "bad encode_image arguments");
  if (pix_fmt != CLIPX_PIX_F32_NCHW && pix_fmt != CLIPX_PIX_U8_NHWC) return fail(CLIPX_E_ARG, "unknown pixel format");
  if (B == 0) return CLIPX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  return host_sync(h, KIND_IMAGE, (const char*)pixels, pix_bytes_per_image(h->desc, pix_fmt), B, pix_fmt, out16, out32);
}
static int encode_text_host(clipx_handle* h, const int32_t* ids, int B, uint16_t* out16, float* out32) {
  if (!h || (B > 0 && (!ids || (!out16 && !out32))) || B < 0) return fail(CLIPX_E_ARG, "bad encode_text arguments");
  if (B == 0) return CLIPX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  return host_sync(h, KIND_TEXT, (const char*)ids, (size_t)h->desc.ctx_len * sizeof(int32_t), B, 0, out16, out32);
}

extern "C" int clipx_encode_image(clipx_handle* h, const void* pixels, int B, int pix_fmt, uint16_t* out_f16) {
  return encode_image_host(h, pixels, B, pix_fmt, out_f16, nullptr);
}
extern "C" int clipx_encode_text(clipx_handle* h, const int32_t* ids, int B, uint16_t* out_f16) {
  return encode_text_host(h, ids, B, out_f16, nullptr);
}
extern "C" int clipx_encode_image_f32(clipx_handle* h, const void* pixels, int B, int pix_fmt, float* out_f32) {
  return encode_image_host(h, pixels, B, pix_fmt, nullptr, out_f32);
}
extern "C" int clipx_encode_text_f32(clipx_handle* h, const int32_t* ids, int B, float* out_f32) {
  return encode_text_host(h, ids, B, nullptr, out_f32);
}

static int encode_async(clipx_handle* h, int kind, const void* in, size_t in_bytes_per_item, int B, int pix_fmt, uint16_t* out_f16,
                        clipx_ticket** ticket) {
  if (!h || !in || !out_f16 || !ticket || B <= 0) return fail(CLIPX_E_ARG, "bad encode_*_async arguments");
  *ticket = nullptr;
  if (B > h->max_batch) return fail(CLIPX_E_ARG, "an asynchronous call takes at most clipx_max_batch() samples");
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  const int s = slot_submit(h, kind, B == 1, (const char*)in, in_bytes_per_item, B, pix_fmt, false);
  if (s < 0) return s;
  *ticket = new clipx_ticket{h, s, B, out_f16, nullptr};
  return CLIPX_OK;
}
extern "C" int clipx_encode_image_async(clipx_handle* h, const void* pixels, int B, int pix_fmt, uint16_t* out_f16,
                                        clipx_ticket** ticket) {
  if (pix_fmt != CLIPX_PIX_F32_NCHW && pix_fmt != CLIPX_PIX_U8_NHWC) return fail(CLIPX_E_ARG, "unknown pixel format");
  return encode_async(h, KIND_IMAGE, pixels, h ? pix_bytes_per_image(h->desc, pix_fmt) : 0, B, pix_fmt, out_f16, ticket);
}
extern "C" int clipx_encode_text_async(clipx_handle* h, const int32_t* ids, int B, uint16_t* out_f16, clipx_ticket** ticket) {
  return encode_async(h, KIND_TEXT, ids, h ? (size_t)h->desc.ctx_len * sizeof(int32_t) : 0, B, 0, out_f16, ticket);
}
extern "C" int clipx_wait(clipx_ticket* t) {
  if (!t) return fail(CLIPX_E_ARG, "ticket is null");
  clipx_handle* h = t->h;
  int r;
  {
    // the event wait runs outside the lock (other threads may submit meanwhile); the slot is this ticket's alone
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipEventSynchronize(h->slots.done[t->slot]);
    std::lock_guard<std::mutex> lk(h->mu);
    r = e == hipSuccess ? slot_collect(h, t->slot, t->nb, t->out16, t->out32)
                        : (h->slots.busy[t->slot] = false, fail(CLIPX_E_HIP, std::string("clipx_wait: ") + hipGetErrorString(e)));
  }
  delete t;
  return r;
}
