// clipx_host.h -- shared by the HOST translation units of the encode half (clipx_api / clipx_encode / clipx_host_path /
// clipx_hooks / bertx_api / preprocess / jpeg_kernels / jpeg_huff_kernels .hip): the one error channel of clipx_last_error(), the device-open helper,
// the pieces both encoder handles are built from (int-slot ring, range guard, workspace gate), the CLIP handle with its state
// grouped by concern, the per-call state, and the handful of functions one file calls in another.
//
// Allocation rule (knnx_host.h): every group has ONE alloc() that leaves the whole group allocated or leaves it EMPTY and returns
// the hipError_t.  Nothing is freed by hand: every member of a handle is an owner (hip_owners.h), a handle goes by `delete`, and a
// create that fails half-way cleans up by that same path.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/clipx.h"
#include "clip_kernels.h"
#include "clipx_ragged_plan.h"
#include "hip_owners.h"

#pragma GCC visibility push(hidden)  // nothing below is part of the library's ABI

namespace clipx {

inline thread_local std::string g_err;  // clipx_last_error()
inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess)                                                                 \
      return clipx::fail(_e == hipErrorOutOfMemory ? CLIPX_E_NOMEM : CLIPX_E_HIP,         \
                         std::string(#expr) + ": " + hipGetErrorString(_e));              \
  } while (0)

// What both *_create functions do first: the device exists, is made current and is a gfx950; *n_cu = its compute units.
inline int open_device(int device, int* n_cu) {
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(CLIPX_E_ARG, "no such HIP device");
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return fail(CLIPX_E_UNSUPPORTED, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);
  *n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  return 0;
}
inline int env_positive(const char* name, int dflt) {  // CLIPX_MAX_BATCH, CLIPX_HOST_CHUNK
  const char* v = getenv(name);
  return v && atoi(v) > 0 ? atoi(v) : dflt;
}
inline bool stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
  return cs != hipStreamCaptureStatusNone;
}

// ---- pieces both handles hold ---------------------------------------------------------------------------------------------
// The f32 blob as uploaded and the matrices converted from it; everything else a model knows of its weights is a pointer into
// these.  Filled while the blob is carved (no alloc() of its own: a carve that fails ends in `delete handle`).
struct Weights {
  DevBuf<float> blob;
  std::vector<DevBuf<char>> mats;
  hipError_t upload(const float* host, size_t floats) {
    hipError_t e = blob.alloc(floats);
    return e != hipSuccess ? e : hipMemcpy(blob, host, floats * sizeof(float), hipMemcpyHostToDevice);
  }
  template <class T>
  hipError_t take(T** p, size_t n) {
    mats.emplace_back();
    hipError_t e = mats.back().alloc(n * sizeof(T));
    *p = reinterpret_cast<T*>(mats.back().p);
    return e;
  }
};

// Ring of page-locked + device int buffers with an event each: per-call host data (the description of a ragged batch) is built in
// a slot, uploaded from it, and the slot is taken again only when the event behind that upload has passed.
struct IntRing {
  static constexpr int N = 4;
  PinBuf host[N];
  DevBuf<int> dev[N];
  Event ev[N];
  bool used[N] = {};
  int next = 0;
  hipError_t alloc(size_t ints) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < N; ++i) {
      if (e == hipSuccess) e = host[i].ensure(ints * sizeof(int));
      dev_alloc(e, dev[i], ints);
      if (e == hipSuccess) e = ev[i].create(hipEventDisableTiming);
    }
    for (int i = 0; i < N && e != hipSuccess; ++i) host[i].reset(), dev[i].reset(), ev[i] = Event();
    return e;
  }
  int* ints(int s) const { return static_cast<int*>(host[s].p); }
  int take(int* s) {
    *s = next;
    next = (next + 1) % N;
    if (used[*s]) HIPCHK(hipEventSynchronize(ev[*s]));  // the upload that last read this slot's host buffer is done
    return 0;
  }
  int upload(int s, size_t n, hipStream_t st) {  // the first n ints of slot s, and the event behind them
    HIPCHK(hipMemcpyAsync(dev[s], host[s], n * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ev[s], st));
    used[s] = true;
    return 0;
  }
};

// Range guard of the fp16 residual stream (clipx.h, CLIPX_E_RANGE): device flags raised by rowstats_kernel / tail_proj_kernel /
// postln_f16_kernel when a row of the stream holds inf / NaN, and their page-locked mirror, which a flag is read back into with the
// results of the call that reports to it (or by the *_range_check entry points).
struct RangeGuard {
  DevBuf<int> flags;
  PinBuf mirror;
  hipError_t alloc(int n, hipStream_t st) {
    hipError_t e = flags.alloc(n);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, n * sizeof(int), st);
    if (e == hipSuccess) e = mirror.ensure(n * sizeof(int));
    if (e == hipSuccess) memset(mirror, 0, n * sizeof(int));
    else flags.reset(), mirror.reset();
    return e;
  }
  int* flag(int i) const { return flags.p + i; }
  int read_back(int i, hipStream_t st) {  // enqueues: flag i -> its mirror, then cleared on the device
    HIPCHK(hipMemcpyAsync(static_cast<int*>(mirror.p) + i, flags.p + i, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemsetAsync(flags.p + i, 0, sizeof(int), st));
    return 0;
  }
  bool test_and_clear(int i) {  // the mirror, once the read-back has completed
    int& m = static_cast<int*>(mirror.p)[i];
    const bool raised = m != 0;
    m = 0;
    return raised;
  }
  static int overflow() {
    return fail(CLIPX_E_RANGE,
                "the residual stream left the range of IEEE fp16 (|x| > 65504 became inf) for at least one row of this batch: these "
                "weights cannot be served by the fp16-stream encoder; the embeddings written for this call must be discarded");
  }
  int check(int i, hipStream_t st) {  // the *_range_check entry points: synchronises st
    if (int r = read_back(i, st)) return r;
    HIPCHK(hipStreamSynchronize(st));
    return test_and_clear(i) ? overflow() : CLIPX_OK;
  }
};

// The activation workspace of a handle is shared by every call: a launch sequence first waits for the event the previous one
// recorded, whichever stream that ran on (callers of the *_device entry points may bring their own streams).  A caller that
// captures `st` into its own hipGraph: the event must not be recorded inside the capture (an event recorded there cannot be waited
// for by a later, non-captured call).  The captured launches are ordered by the graph itself; the caller must not replay it
// concurrently with other calls on this handle (clipx.h).
struct WsGate {
  Event ev;
  bool valid = false;
  hipError_t alloc() { return ev.create(hipEventDisableTiming); }
  int acquire(hipStream_t st) {
    if (valid && !stream_is_capturing(st)) HIPCHK(hipStreamWaitEvent(st, ev, 0));
    return 0;
  }
  int release(hipStream_t st) {
    if (stream_is_capturing(st)) return 0;
    HIPCHK(hipEventRecord(ev, st));
    valid = true;
    return 0;
  }
};

// ---- the CLIP encoder handle ------------------------------------------------------------------------------------------------
struct LayerW {
  const float *ln1_w, *ln1_b, *qkv_b, *out_b, *ln2_w, *ln2_b, *fc1_b, *fc2_b;  // into the f32 device blob
  bf16 *qkv_w, *out_w, *fc1_w, *fc2_w;                                          // bf16 copies
  // ln_1 is folded into the QKV projection and ln_2 into fc1 (fold_layernorm): qkv_w / fc1_w hold
  // fp16(W gamma - rowmean(W gamma)) (IEEE fp16 bits behind the bf16-typed pointer) and these are bias + W beta; the GEMM
  // reads the fp16 residual stream itself and its epilogue multiplies by the row's 1/std (launch_rowstats)
  float *qkv_c, *fc1_c;
};

struct Tower {
  int width = 0, layers = 0, heads = 0, mlp = 0, T = 0;
  std::vector<LayerW> L;
  const float *lnf_w = nullptr, *lnf_b = nullptr;  // ln_post / ln_final
  bf16* proj = nullptr;                            // [embed, width]
};

struct ClipWeights : Weights {
  Tower vis, txt;
  int Kp = 0, PP3 = 0;
  bf16* conv_w = nullptr;   // [v_width, Kp]
  float* clspos = nullptr;  // [T_v, v_width]: row 0 = class + pos[0], row t = pos[t]
  const float *ln_pre_w = nullptr, *ln_pre_b = nullptr;
  const float *tok_emb = nullptr, *txt_pos = nullptr;
};

// activation workspace (shared by both towers)
struct Workspace {
  DevBuf<float> x;     // f32 [rows, width]: the patch-embedding output in front of ln_pre (vision tower only)
  DevBuf<float> rstd;  // [rows] LayerNorm 1/std of the current residual rows
  // xn = THE residual stream, IEEE fp16 [rows, width] (fp16 bits behind the bf16-typed pointer): read as the A operand of the
  // LayerNorm-folded GEMMs (QKV, fc1) and updated in place by the residual epilogues of out_proj / fc2.  Round 3: it replaced
  // an f32 stream + bf16 shadow (673 MB -> 269 MB moved per residual GEMM at ViT-L/14 bs 256; same accuracy: the stream has
  // 3 mantissa bits more than the bf16 operands it used to be rounded to).
  DevBuf<bf16> xn, qkv, att, hbuf, patches;
  DevBuf<float> splitk;  // partial products of the small-M split-K GEMMs (gemm128.hip)
  size_t splitk_bytes = 0;
  // text rows: a ragged batch is padded to whole 256-row m-tiles (clipx_ragged_plan.h), at most 255 rows past a full rectangular one
  hipError_t alloc(size_t Bm, const Tower& V, const Tower& X, int Kp) {
    const size_t rowsV = Bm * V.T, rowsX = ragged_max_rows(Bm, X.T);
    const size_t nx = std::max(rowsV * V.width, rowsX * X.width);
    hipError_t e = hipSuccess;
    dev_alloc(e, x, rowsV * V.width);
    dev_alloc(e, xn, nx);
    dev_alloc(e, rstd, std::max(rowsV, rowsX));
    dev_alloc(e, qkv, std::max(rowsV * 3 * V.width, rowsX * 3 * X.width));
    dev_alloc(e, att, nx);
    dev_alloc(e, hbuf, std::max(rowsV * V.mlp, rowsX * X.mlp));
    dev_alloc(e, patches, rowsV * Kp);
    dev_alloc(e, splitk, ((size_t)32 << 20) / sizeof(float));
    if (e != hipSuccess) *this = Workspace();
    else splitk_bytes = (size_t)32 << 20;
    return e;
  }
};

// Host hand-over: staging slots (pinned in/out + device in/out); a slot carries one chunk from its upload to the moment its
// result has been copied to the caller (synchronous calls pipeline their chunks through them; every asynchronous ticket owns one)
struct StagingSlots {
  static constexpr int N = 4;
  PinBuf pin_in[N], pin_out[N];  // pin_out: f16 [max_batch, E] then f32 [max_batch, E]
  DevBuf<char> dev_in[N];
  DevBuf<uint16_t> dev_out[N];
  DevBuf<float> dev_out32[N];
  Event copied[N], done[N];
  bool busy[N] = {};
  int next = 0;
  size_t in_bytes = 0, out_bytes = 0;
  hipError_t alloc(size_t in_bytes_, size_t out_rows_x_E) {
    in_bytes = in_bytes_;
    out_bytes = out_rows_x_E * sizeof(uint16_t);
    hipError_t e = hipSuccess;
    for (int s = 0; s < N; ++s) {
      if (e == hipSuccess) e = pin_in[s].ensure(in_bytes);
      if (e == hipSuccess) e = pin_out[s].ensure(out_bytes * 3);
      dev_alloc(e, dev_in[s], in_bytes);
      dev_alloc(e, dev_out[s], out_rows_x_E);
      dev_alloc(e, dev_out32[s], out_rows_x_E);
      if (e == hipSuccess) e = copied[s].create(hipEventDisableTiming);
      if (e == hipSuccess) e = done[s].create(hipEventDisableTiming);
    }
    for (int s = 0; s < N && e != hipSuccess; ++s) {
      pin_in[s].reset(), pin_out[s].reset(), dev_in[s].reset(), dev_out[s].reset(), dev_out32[s].reset();
      copied[s] = Event(), done[s] = Event();
    }
    return e;
  }
};

// Small batches (the B = 1 query encode of KnnService.compute_query, clip_back.py:207-255) are ~170 dependent launches of
// 5-15 us kernels: their launch sequence is captured once per (tower, B, buffers, stream) into a hipGraph and replayed.
struct GraphCache {
  typedef std::tuple<int, int, int, const void*, const void*, const void*, hipStream_t> Key;
  std::map<Key, GraphExec> execs;
  std::map<Key, int> seen;  // a launch sequence is captured the SECOND time its key shows up: a caller that brings fresh
                            // buffers on every call (new addresses) never pays for captures it cannot reuse
  bool on = true;
};

// One bracketed launch scope.  Marker form: ev[0] / ev[1] are recorded on the stream in front of and behind the scope's launches.
// Stamp form (GEMMs): every kernel of the scope was given a slot of its own and wrote its first start and last end into it; the
// scope's time is the sum over its kernels of last_end - first_start -- never an interval across kernels.
struct ProfEvent {
  hipEvent_t ev[2];   // marker form
  bool stamps;        // stamp form: the scope's slots are the ids slot0 .. slot0 + nslots - 1 (scopes do not interleave: h->mu)
  int slot0, nslots;
  hipStream_t st;     // the stream the scope's launches went to
  int kind;
  double flops;
};

constexpr int PROF_CHUNK_SLOTS = 8192;  // slots per device chunk (8 MiB): 55 ViT-L/14 steps of 147 GEMM kernels between two clipx_profile_get

struct Profiler {
  int mask = 0;          // bit k set: launches of kind k (0 gemm, 1 attention, 2 layernorm, 3 other) are bracketed
  bool markers = false;  // CLIPX_OPT_PROF_MARKERS: the marker form for the GEMMs as well (default: the kernels' own clock stamps)
  std::vector<Event> created;      // every timing event made so far (clipx_profile_events); the two below borrow from it
  std::vector<hipEvent_t> unused;  // free for reuse: clipx_profile_get hands back what it has read
  std::vector<ProfEvent> scopes;
  // stamp form: the slots live in device chunks of PROF_CHUNK_SLOTS; `book` counts the ids handed out since the last read
  StampBook book{PROF_CHUNK_SLOTS};
  std::vector<DevBuf<StampSlot>> chunks;
  std::vector<StampSlot> host;  // where clipx_profile_get reads the slots back to, indexed by slot id
  int clock_khz = 0;            // hipDeviceAttributeWallClockRate, read once
  bool starved = false;         // the slots ran out and no further chunk could be allocated: some kernel ran without a slot
  StampSlot* slot(int id) const { return chunks[id / PROF_CHUNK_SLOTS].p + id % PROF_CHUNK_SLOTS; }
  // one more chunk, filled on `st` and synchronised before its ids exist: whichever stream a later scope launches on, the fill
  // has run (a scope that runs out of slots pays that wait once per 8 192 kernels; clipx_profile_enable pays it for the first chunk)
  hipError_t add_chunk(hipStream_t st) {
    DevBuf<StampSlot> c;
    hipError_t e = c.alloc(PROF_CHUNK_SLOTS);
    if (e == hipSuccess) e = launch_fill_stamps(c, PROF_CHUNK_SLOTS, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    chunks.push_back(std::move(c));
    book.add_chunk();
    return hipSuccess;
  }
};

}  // namespace clipx

struct clipx_handle {
  clipx_model_desc desc{};
  int device = 0;
  int max_batch = 256;
  int host_chunk = 256;  // chunk of the host-buffer pipeline (H2D of chunk i+1 overlaps the kernels of chunk i); measured
                         // at B=256: chunks of 32/64/128/256 -> 92/65/58/56.5 ms, small chunks lose more GEMM efficiency than
                         // the overlap wins
  int gemm_variant = clipx::GEMM_V_DEFAULT;  // 6: the 4-wave 256x256 kernel (gemm256w4.hip) where it has the form, the 8-wave one (variant 3) elsewhere
  int n_cu = 256;
  bool pool_last_block = true;  // last block past the attention on the pooled rows only (CLIPX_FULL_LAST_BLOCK=1: all rows)
  // LayerNorm statistics of the folded GEMMs inside the 4-wave GEMM kernel instead of a pass of their own: CLIPX_LN_FUSED=1, OFF by
  // default -- measured 50.5 ms per ViT-L/14 step against 42.6 (profiles/r06o_ab_ln_fused.log): the 128 v_dot2_f32_f16 per K-tile do
  // not hide behind the MFMAs of a one-wave-per-SIMD kernel (~8 cycles of issue each), they cost 8 ms to save 1.2
  bool ln_fused = false;
  // Ragged text tower (CLIPX_RAGGED_TEXT=0: off).  The text transformer is causal and the embedding is read at the EOT token:
  // rows after a caption's EOT influence nothing that is read, so batches above the hipGraph sizes run every layer on
  // sum(eot_i + 1) rows instead of B x ctx_len.  Per call: lens / offsets / row map / pooled rows, built on the host from the
  // token ids in a slot of `ragged`.
  bool ragged_text = true;
  int last_text_rows = 0;  // rows the latest text chunk ran its layers on (clipx_last_text_rows)
  std::mutex mu;

  // Members are destroyed bottom-up: the streams are declared first, so that every buffer, event and graph exec below is gone
  // before the streams it was used on (clipx_destroy has synchronised them).
  Stream stream, copy_stream;
  clipx::ClipWeights w;
  clipx::Workspace ws;
  clipx::WsGate gate;
  clipx::StagingSlots slots;
  clipx::IntRing ragged;
  PinBuf ids_back;          // device-pointer calls: the ids come back through this page-locked buffer
  clipx::RangeGuard range;  // one flag per staging slot + one for the *_device entry points (index StagingSlots::N)
  clipx::GraphCache graphs;
  clipx::Profiler prof;
};

namespace clipx {

// What one API call hands down to everything it launches (never parked on the handle).
struct Call {
  hipStream_t st;
  bool single_query;        // the API call is ONE sample (not per chunk: the last chunk of a 7-sample call is one sample too, and
                            // must equal its row of an unchunked call)
  int* range_flag;          // the device flag this call's launches report to
  const int32_t* ids_host;  // text: the caller's host copy of the chunk's ids, or null (the ragged tower reads them back)
};

enum { KIND_IMAGE = 0, KIND_TEXT = 1 };

inline size_t pix_bytes_per_image(const clipx_model_desc& d, int fmt) {
  const size_t px = (size_t)3 * d.image_size * d.image_size;
  return fmt == CLIPX_PIX_F32_NCHW ? px * sizeof(float) : px;
}

// clipx_encode.hip: one chunk (B <= max_batch), everything on the device, asynchronous on c.st
int vision_chunk(clipx_handle* h, const Call& c, const void* pix_dev, int B, int fmt, uint16_t* out_f16, float* out_f32);
int text_chunk(clipx_handle* h, const Call& c, const int32_t* ids_dev, int B, uint16_t* out_f16, float* out_f32);
// launch_gemm(g) on st as ONE profiled scope of `flops` (g.events is set here); the caller holds h->mu
int profiled_gemm(clipx_handle* h, GemmArgs& g, hipStream_t st, double flops);

}  // namespace clipx

#pragma GCC visibility pop
