// bertx_api.hip -- host side of the clipx_bert_* part of include/clipx.h: the multilingual text towers of the reference's
// `use_mclip` (clip_inference/mapper.py:44-47, 62-63: SentenceTransformer(...).encode; clip_back.py:837-859: M-CLIP's XLM-R +
// LinearTransformation), one post-LN BERT-family encoder on the CLIP encoder's GEMMs and ragged attention plus the three kernels
// of bert_kernels.hip.  A batch is always ragged: sample b owns lens[b] packed rows, padded to whole 256-row GEMM tiles with
// pseudo-samples the way ragged_prepare (clipx_api.hip) pads the CLIP text tower.  No hipGraphs, no CPU compute path.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/clipx.h"
#include "bert_kernels.h"
#include "clip_kernels.h"

using namespace clipx;

extern "C" int clipx_set_error(int code, const char* msg);  // clipx_api.hip: the thread-local message of clipx_last_error()

static int bfail(int code, const std::string& msg) { return clipx_set_error(code, msg.c_str()); }
#define BHIPCHK(expr)                                                                      \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return bfail(_e == hipErrorOutOfMemory ? CLIPX_E_NOMEM : CLIPX_E_HIP,                \
                   std::string(#expr) + ": " + hipGetErrorString(_e));                     \
  } while (0)

namespace {

constexpr int BERT_PAD_MAX = 255;   // most rows a chunk is padded by (whole 256-row m-tiles)
constexpr int BERT_MAX_LEN = 128;   // the ragged attention kernels: head dimension 64, at most 128 tokens

struct BertLayer {
  const float *qkv_b, *out_b, *ln_att_w, *ln_att_b, *fc1_b, *fc2_b, *ln_out_w, *ln_out_b;  // into the f32 device blob
  bf16 *qkv_w, *fc1_w;  // IEEE fp16 bits behind the bf16-typed pointer: the GEMMs whose A operand is the fp16 stream
  bf16 *out_w, *fc2_w;  // bf16: the GEMMs whose A operand is the attention output / the GELU output
};

}  // namespace

struct clipx_bert {
  clipx_bert_desc desc{};
  int device = 0;
  int max_batch = 256;
  int n_cu = 256;
  std::mutex mu;
  hipStream_t stream = nullptr;

  float* blob_dev = nullptr;
  std::vector<void*> owned;
  const float *word = nullptr, *pos = nullptr, *ln_emb_w = nullptr, *ln_emb_b = nullptr, *dense_w = nullptr, *dense_b = nullptr;
  std::vector<BertLayer> L;

  // activation workspace: x = the residual stream, IEEE fp16 [rows, width]
  bf16 *x = nullptr, *qkv = nullptr, *att = nullptr, *hbuf = nullptr;
  float* ones = nullptr;   // [rows] row scales of the fp16-operand GEMMs (no LayerNorm is folded into them here)
  float* y_raw = nullptr;  // [max_batch, out_dim] the dense layer's output in front of the norm
  int max_rows = 0, max_samples = 0;

  // Per chunk: src / lens / offs of its samples and pseudo-samples (and, for host callers, the ids), built on the host and uploaded
  // from a ring of page-locked slots; a slot is reused when the event behind its upload has passed.
  static constexpr int NSLOT = 4;
  int* slot_host[NSLOT] = {};
  int* slot_dev[NSLOT] = {};
  hipEvent_t slot_ev[NSLOT] = {};
  bool slot_used[NSLOT] = {};
  int slot_next = 0;

  float* out32_dev = nullptr;  // host-pointer calls: the chunk's results on their way back
  uint16_t* out16_dev = nullptr;
  void* out_host = nullptr;    // page-locked: f32 [max_batch, E] then f16 [max_batch, E]
  int* range_flag = nullptr;   // device; raised by postln_f16_kernel when a row of the stream holds inf / NaN
  int* range_host = nullptr;   // page-locked
  hipEvent_t ev_ws = nullptr;  // the workspace is shared by every call, whichever stream it runs on
  bool ev_ws_valid = false;
};

static int bert_alloc(clipx_bert* h, void** p, size_t bytes) {
  BHIPCHK(hipMalloc(p, bytes));
  h->owned.push_back(*p);
  return 0;
}

extern "C" size_t clipx_bert_blob_floats(const clipx_bert_desc* d) {
  if (!d) return 0;
  const size_t w = d->width, mlp = d->mlp, E = d->out_dim;
  const size_t layer = 3 * w * w + 3 * w + w * w + w + 2 * w + mlp * w + mlp + w * mlp + w + 2 * w;
  return (size_t)d->vocab * w + (size_t)d->max_pos * w + 2 * w + (size_t)d->layers * layer + E * w + (d->dense_bias ? E : 0);
}

static int bert_check_desc(const clipx_bert_desc* d) {
  if (d->width <= 0 || d->width % 128 || d->width > 2048) return bfail(CLIPX_E_UNSUPPORTED, "width must be a multiple of 128, at most 2048");
  if (d->heads <= 0 || d->width % d->heads) return bfail(CLIPX_E_ARG, "width must be a multiple of heads");
  if (d->width / d->heads != 64) return bfail(CLIPX_E_UNSUPPORTED, "the ragged attention kernels of this build need head dimension 64");
  if (d->max_len > BERT_MAX_LEN) return bfail(CLIPX_E_UNSUPPORTED, "texts of more than 128 tokens have no ragged attention kernel");
  if (d->mlp <= 0 || d->mlp % 128) return bfail(CLIPX_E_UNSUPPORTED, "mlp width must be a multiple of 128");
  if (d->max_len < 1 || d->layers <= 0 || d->vocab <= 0 || d->out_dim <= 0) return bfail(CLIPX_E_ARG, "bad layer / vocab / length / out_dim");
  if (d->pos_offset < 0 || d->pos_offset + d->max_len > d->max_pos) return bfail(CLIPX_E_ARG, "pos_offset + max_len exceeds the position table");
  if (!(d->ln_eps > 0.f)) return bfail(CLIPX_E_ARG, "ln_eps must be positive");
  return 0;
}

static int bert_create_impl(clipx_bert* h, const float* blob, size_t blob_floats) {
  const clipx_bert_desc& d = h->desc;
  const size_t w = d.width, mlp = d.mlp, E = d.out_dim;
  BHIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  BHIPCHK(hipMalloc((void**)&h->blob_dev, blob_floats * sizeof(float)));
  BHIPCHK(hipMemcpy(h->blob_dev, blob, blob_floats * sizeof(float), hipMemcpyHostToDevice));
  int r;
  float* p = h->blob_dev;
  h->word = p; p += (size_t)d.vocab * w;
  h->pos = p; p += (size_t)d.max_pos * w;
  h->ln_emb_w = p; p += w;
  h->ln_emb_b = p; p += w;
  h->L.resize(d.layers);
  for (int l = 0; l < d.layers; ++l) {
    BertLayer& L = h->L[l];
    const float* qkv32 = p; p += 3 * w * w;
    L.qkv_b = p; p += 3 * w;
    const float* out32 = p; p += w * w;
    L.out_b = p; p += w;
    L.ln_att_w = p; p += w;
    L.ln_att_b = p; p += w;
    const float* fc1_32 = p; p += mlp * w;
    L.fc1_b = p; p += mlp;
    const float* fc2_32 = p; p += w * mlp;
    L.fc2_b = p; p += w;
    L.ln_out_w = p; p += w;
    L.ln_out_b = p; p += w;
    if ((r = bert_alloc(h, (void**)&L.qkv_w, 3 * w * w * 2))) return r;
    if ((r = bert_alloc(h, (void**)&L.out_w, w * w * 2))) return r;
    if ((r = bert_alloc(h, (void**)&L.fc1_w, mlp * w * 2))) return r;
    if ((r = bert_alloc(h, (void**)&L.fc2_w, w * mlp * 2))) return r;
    // the existing GEMMs take fp16 x fp16 (A = the fp16 stream) and bf16 x bf16: the weights are converted once, here
    BHIPCHK(launch_f32_to_f16(qkv32, L.qkv_w, (int64_t)(3 * w * w), h->stream));
    BHIPCHK(launch_f32_to_bf16(out32, L.out_w, (int64_t)(w * w), h->stream));
    BHIPCHK(launch_f32_to_f16(fc1_32, L.fc1_w, (int64_t)(mlp * w), h->stream));
    BHIPCHK(launch_f32_to_bf16(fc2_32, L.fc2_w, (int64_t)(w * mlp), h->stream));
  }
  h->dense_w = p; p += E * w;
  if (d.dense_bias) { h->dense_b = p; p += E; }
  if ((size_t)(p - h->blob_dev) != blob_floats) return bfail(CLIPX_E_ARG, "internal: blob carve does not match clipx_bert_blob_floats");

  const size_t Bm = h->max_batch;
  const size_t rows = Bm * d.max_len + BERT_PAD_MAX;
  h->max_rows = (int)rows;
  h->max_samples = (int)Bm + BERT_PAD_MAX;  // a pseudo-sample owns one pad row at least
  if ((r = bert_alloc(h, (void**)&h->x, rows * w * 2))) return r;
  if ((r = bert_alloc(h, (void**)&h->qkv, rows * 3 * w * 2))) return r;
  if ((r = bert_alloc(h, (void**)&h->att, rows * w * 2))) return r;
  if ((r = bert_alloc(h, (void**)&h->hbuf, rows * mlp * 2))) return r;
  if ((r = bert_alloc(h, (void**)&h->ones, rows * sizeof(float)))) return r;
  BHIPCHK(launch_fill_f32(h->ones, 1.f, (int64_t)rows, h->stream));
  if ((r = bert_alloc(h, (void**)&h->y_raw, Bm * E * sizeof(float)))) return r;
  if ((r = bert_alloc(h, (void**)&h->out32_dev, Bm * E * sizeof(float)))) return r;
  if ((r = bert_alloc(h, (void**)&h->out16_dev, Bm * E * sizeof(uint16_t)))) return r;
  BHIPCHK(hipHostMalloc(&h->out_host, Bm * E * (sizeof(float) + sizeof(uint16_t)), hipHostMallocDefault));
  const size_t slot_ints = 3 * (size_t)h->max_samples + Bm * d.max_len;
  for (int s = 0; s < clipx_bert::NSLOT; ++s) {
    BHIPCHK(hipHostMalloc((void**)&h->slot_host[s], slot_ints * sizeof(int), hipHostMallocDefault));
    if ((r = bert_alloc(h, (void**)&h->slot_dev[s], slot_ints * sizeof(int)))) return r;
    BHIPCHK(hipEventCreateWithFlags(&h->slot_ev[s], hipEventDisableTiming));
  }
  if ((r = bert_alloc(h, (void**)&h->range_flag, sizeof(int)))) return r;
  BHIPCHK(hipMemsetAsync(h->range_flag, 0, sizeof(int), h->stream));
  BHIPCHK(hipHostMalloc((void**)&h->range_host, sizeof(int), hipHostMallocDefault));
  *h->range_host = 0;
  BHIPCHK(hipEventCreateWithFlags(&h->ev_ws, hipEventDisableTiming));
  BHIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int clipx_bert_create(const clipx_bert_desc* desc, const float* blob, size_t blob_floats, int device, clipx_bert** out) {
  if (!desc || !blob || !out) return bfail(CLIPX_E_ARG, "null argument");
  *out = nullptr;
  int r = bert_check_desc(desc);
  if (r) return r;
  if (blob_floats != clipx_bert_blob_floats(desc)) return bfail(CLIPX_E_ARG, "weight blob has the wrong number of floats for this model description");
  int ndev = 0;
  BHIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return bfail(CLIPX_E_ARG, "no such HIP device");
  BHIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  BHIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return bfail(CLIPX_E_UNSUPPORTED, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);
  clipx_bert* h = new clipx_bert();
  h->desc = *desc;
  h->device = device;
  const char* mb = getenv("CLIPX_MAX_BATCH");
  if (mb && atoi(mb) > 0) h->max_batch = atoi(mb);
  h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  r = bert_create_impl(h, blob, blob_floats);
  if (r) {
    const std::string keep = clipx_last_error();
    clipx_bert_destroy(h);
    return bfail(r, keep);
  }
  *out = h;
  return CLIPX_OK;
}

extern "C" void clipx_bert_destroy(clipx_bert* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : h->owned) (void)hipFree(p);
  if (h->blob_dev) (void)hipFree(h->blob_dev);
  for (int s = 0; s < clipx_bert::NSLOT; ++s) {
    if (h->slot_host[s]) (void)hipHostFree(h->slot_host[s]);
    if (h->slot_ev[s]) (void)hipEventDestroy(h->slot_ev[s]);
  }
  if (h->out_host) (void)hipHostFree(h->out_host);
  if (h->range_host) (void)hipHostFree(h->range_host);
  if (h->ev_ws) (void)hipEventDestroy(h->ev_ws);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int clipx_bert_out_dim(const clipx_bert* h) { return h ? h->desc.out_dim : 0; }

static int bert_gemm(clipx_bert* h, hipStream_t st, const bf16* A, const bf16* W, const float* bias, void* out, int M, int N, int K, int epi,
                     bool f16) {
  GemmArgs g{};
  g.A = A; g.W = W; g.bias = bias; g.out = out; g.T = 1;
  g.M = M; g.N = N; g.K = K; g.epi = epi; g.variant = 6; g.n_cu = h->n_cu;
  g.rowscale = f16 ? h->ones : nullptr;
  g.f16 = f16 ? 1 : 0;
  BHIPCHK(launch_gemm(g, st));
  return 0;
}

static int bert_take_slot(clipx_bert* h, int* slot) {
  const int s = h->slot_next;
  h->slot_next = (s + 1) % clipx_bert::NSLOT;
  if (h->slot_used[s]) BHIPCHK(hipEventSynchronize(h->slot_ev[s]));
  *slot = s;
  return 0;
}

// One chunk (nb <= max_batch samples whose lengths were checked), everything on the device, asynchronous on `st`.  ids_dev: int32
// [nb, max_len].  Slot `s` is the caller's (bert_take_slot); its event is recorded here, behind the upload of the description.
static int bert_chunk(clipx_bert* h, hipStream_t st, int s, const int32_t* ids_dev, const int32_t* lens_host, int nb, float* out32,
                      uint16_t* out16) {
  const clipx_bert_desc& d = h->desc;
  const int w = d.width;
  // layout of the slot: src [S], lens [S], offs [S]  (S is known once every length is)
  int* host = h->slot_host[s];
  int M = 0, longest = 0;
  for (int b = 0; b < nb; ++b) {
    if (lens_host[b] > lens_host[longest]) longest = b;
    M += lens_host[b];
  }
  const int lmax = lens_host[longest];
  const int Mp = gemm256_whole_tile_rows(M, 3 * w, w, 6, h->n_cu);
  const int S = nb + (Mp - M + lmax - 1) / lmax;
  if (Mp > h->max_rows || S > h->max_samples) return bfail(CLIPX_E_ARG, "internal: the activation workspace does not hold the padded rows");
  int *src = host, *lens = host + S, *offs = host + 2 * S;
  // The pad rows belong to pseudo-samples that repeat a prefix of the longest text: finite rows of the model's own making for the
  // GEMM tiles to chew on (nothing a GEMM reads is uninitialised), never read by a real row -- attention stays inside a sample
  // and every other kernel is row-wise -- and never pooled.
  for (int b = 0, m = 0, left = Mp - M; b < S; ++b) {
    src[b] = b < nb ? b : longest;
    lens[b] = b < nb ? lens_host[b] : std::min(lmax, left);
    if (b >= nb) left -= lens[b];
    offs[b] = m;
    m += lens[b];
  }
  int* dev = h->slot_dev[s];
  BHIPCHK(hipMemcpyAsync(dev, host, (size_t)3 * S * sizeof(int), hipMemcpyHostToDevice, st));
  BHIPCHK(hipEventRecord(h->slot_ev[s], st));
  h->slot_used[s] = true;
  const int *src_d = dev, *lens_d = dev + S, *offs_d = dev + 2 * S;

  BHIPCHK(launch_bert_embed(ids_dev, d.max_len, src_d, offs_d, lens_d, S, lmax, Mp, h->word, h->pos, d.pos_offset, h->ln_emb_w, h->ln_emb_b,
                            h->x, w, d.vocab, d.ln_eps, st));
  // Per layer (post-LN: each LayerNorm rewrites the stream, it is both the next GEMM's operand and the next residual):
  //   qkv = fp16(x Wqkv^T + b)                     fp16 MFMA, epilogue 7
  //   att = attention(qkv), not causal, keys of the sample's own rows only
  //   x = fp16(x + att Wout^T + b); x = LN_att(x)  bf16 MFMA, epilogue 6 (f32 add), then postln in place
  //   h = bf16(gelu(x Wfc1^T + b))                 fp16 MFMA, epilogue 2
  //   x = fp16(x + h Wfc2^T + b); x = LN_out(x)    bf16 MFMA, epilogue 6, postln
  int r;
  for (int l = 0; l < d.layers; ++l) {
    const BertLayer& L = h->L[l];
    if ((r = bert_gemm(h, st, h->x, L.qkv_w, L.qkv_b, h->qkv, Mp, 3 * w, w, EPI_BIAS_F16, true))) return r;
    BHIPCHK(launch_attention(h->qkv, h->att, S, lmax, d.heads, 64, 0, st, 0, offs_d, lens_d));
    if ((r = bert_gemm(h, st, h->att, L.out_w, L.out_b, h->x, Mp, w, w, EPI_BIAS_RESID_H16, false))) return r;
    BHIPCHK(launch_postln_f16(h->x, L.ln_att_w, L.ln_att_b, Mp, w, d.ln_eps, h->range_flag, st));
    if ((r = bert_gemm(h, st, h->x, L.fc1_w, L.fc1_b, h->hbuf, Mp, d.mlp, w, EPI_BIAS_GELU_BF16, true))) return r;
    if ((r = bert_gemm(h, st, h->hbuf, L.fc2_w, L.fc2_b, h->x, Mp, w, d.mlp, EPI_BIAS_RESID_H16, false))) return r;
    BHIPCHK(launch_postln_f16(h->x, L.ln_out_w, L.ln_out_b, Mp, w, d.ln_eps, h->range_flag, st));
  }
  BHIPCHK(launch_bert_pool(h->x, offs_d, lens_d, h->dense_w, h->dense_b, h->y_raw, out32, out16, nb, w, d.out_dim, st));
  return 0;
}

static int bert_check_lens(const clipx_bert* h, const int32_t* lens, int B) {
  for (int b = 0; b < B; ++b)
    if (lens[b] < 1 || lens[b] > h->desc.max_len)
      return bfail(CLIPX_E_ARG, "lens[" + std::to_string(b) + "] = " + std::to_string(lens[b]) + " is outside 1 .. max_len = " +
                                    std::to_string(h->desc.max_len));
  return 0;
}

static const char* kBertRangeMsg =
    "the residual stream left the range of IEEE fp16 for at least one row of this batch: these weights cannot be served by the "
    "fp16-stream encoder; the embeddings written for this call must be discarded";

extern "C" int clipx_bert_encode(clipx_bert* h, const int32_t* ids, const int32_t* lens, int B, float* out_f32, uint16_t* out_f16) {
  if (!h || !ids || !lens || !out_f32 || B < 1) return bfail(CLIPX_E_ARG, "bad bert_encode arguments");
  int r = bert_check_lens(h, lens, B);
  if (r) return r;
  std::lock_guard<std::mutex> lk(h->mu);
  BHIPCHK(hipSetDevice(h->device));
  const clipx_bert_desc& d = h->desc;
  const size_t E = d.out_dim;
  hipStream_t st = h->stream;
  if (h->ev_ws_valid) BHIPCHK(hipStreamWaitEvent(st, h->ev_ws, 0));
  bool overflow = false;
  for (int o = 0; o < B; o += h->max_batch) {
    const int nb = std::min(h->max_batch, B - o);
    int s;
    if ((r = bert_take_slot(h, &s))) return r;
    int* ids_pin = h->slot_host[s] + 3 * (size_t)h->max_samples;
    int* ids_dev = h->slot_dev[s] + 3 * (size_t)h->max_samples;
    // rows are copied whole; positions past lens[b] are never read on the device (the embedding kernel's mask)
    memcpy(ids_pin, ids + (size_t)o * d.max_len, (size_t)nb * d.max_len * sizeof(int32_t));
    BHIPCHK(hipMemcpyAsync(ids_dev, ids_pin, (size_t)nb * d.max_len * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((r = bert_chunk(h, st, s, ids_dev, lens + o, nb, h->out32_dev, out_f16 ? h->out16_dev : nullptr))) return r;
    char* po = (char*)h->out_host;
    BHIPCHK(hipMemcpyAsync(po, h->out32_dev, (size_t)nb * E * sizeof(float), hipMemcpyDeviceToHost, st));
    if (out_f16) BHIPCHK(hipMemcpyAsync(po + (size_t)h->max_batch * E * sizeof(float), h->out16_dev, (size_t)nb * E * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    BHIPCHK(hipMemcpyAsync(h->range_host, h->range_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    BHIPCHK(hipMemsetAsync(h->range_flag, 0, sizeof(int), st));
    BHIPCHK(hipStreamSynchronize(st));
    memcpy(out_f32 + (size_t)o * E, po, (size_t)nb * E * sizeof(float));
    if (out_f16) memcpy(out_f16 + (size_t)o * E, po + (size_t)h->max_batch * E * sizeof(float), (size_t)nb * E * sizeof(uint16_t));
    if (*h->range_host) { overflow = true; *h->range_host = 0; }
  }
  BHIPCHK(hipEventRecord(h->ev_ws, st));
  h->ev_ws_valid = true;
  return overflow ? bfail(CLIPX_E_RANGE, kBertRangeMsg) : CLIPX_OK;
}

extern "C" int clipx_bert_encode_device(clipx_bert* h, const int32_t* ids_dev, const int32_t* lens_host, int B, float* out_f32_dev,
                                        uint16_t* out_f16_dev, void* stream) {
  if (!h || !ids_dev || !lens_host || !out_f32_dev || B < 1) return bfail(CLIPX_E_ARG, "bad bert_encode_device arguments");
  int r = bert_check_lens(h, lens_host, B);
  if (r) return r;
  std::lock_guard<std::mutex> lk(h->mu);
  BHIPCHK(hipSetDevice(h->device));
  const clipx_bert_desc& d = h->desc;
  const size_t E = d.out_dim;
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  if (h->ev_ws_valid) BHIPCHK(hipStreamWaitEvent(st, h->ev_ws, 0));
  for (int o = 0; o < B; o += h->max_batch) {
    const int nb = std::min(h->max_batch, B - o);
    int s;
    if ((r = bert_take_slot(h, &s))) return r;
    if ((r = bert_chunk(h, st, s, ids_dev + (size_t)o * d.max_len, lens_host + o, nb, out_f32_dev + (size_t)o * E,
                        out_f16_dev ? out_f16_dev + (size_t)o * E : nullptr)))
      return r;
  }
  BHIPCHK(hipEventRecord(h->ev_ws, st));
  h->ev_ws_valid = true;
  return CLIPX_OK;
}

extern "C" int clipx_bert_range_check(clipx_bert* h, void* stream) {
  if (!h) return bfail(CLIPX_E_ARG, "handle is null");
  std::lock_guard<std::mutex> lk(h->mu);
  BHIPCHK(hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  BHIPCHK(hipMemcpyAsync(h->range_host, h->range_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  BHIPCHK(hipMemsetAsync(h->range_flag, 0, sizeof(int), st));
  BHIPCHK(hipStreamSynchronize(st));
  if (*h->range_host) {
    *h->range_host = 0;
    return bfail(CLIPX_E_RANGE, kBertRangeMsg);
  }
  return CLIPX_OK;
}

// ---------------------------------------------------------------------------------------------
// the three kernels in isolation (per-kernel parity tests)
// ---------------------------------------------------------------------------------------------
static int bert_check_d(int d) {
  if (d <= 0 || d % 128 || d > 2048) return bfail(CLIPX_E_UNSUPPORTED, "d must be a multiple of 128, <= 2048");
  return 0;
}

extern "C" int clipx_bert_embed_device(int device, const int32_t* ids, int ids_stride, const int32_t* offs, const int32_t* lens, int B, int T,
                                       int rows, const float* word, const float* pos, int pos_offset, int max_pos, const float* gamma,
                                       const float* beta, void* out_f16, int d, int vocab, float eps, void* stream) {
  if (!ids || !offs || !lens || !word || !pos || !gamma || !beta || !out_f16 || B <= 0 || rows <= 0 || vocab <= 0)
    return bfail(CLIPX_E_ARG, "bad bert_embed arguments");
  if (T < 1 || pos_offset < 0 || pos_offset + T > max_pos) return bfail(CLIPX_E_ARG, "positions pos_offset .. pos_offset + T - 1 must lie inside the position table");
  if (ids_stride < 0 || (ids_stride > 0 && ids_stride < T)) return bfail(CLIPX_E_ARG, "ids_stride must be 0 (packed ids) or at least T");
  int r = bert_check_d(d);
  if (r) return r;
  BHIPCHK(hipSetDevice(device));
  BHIPCHK(launch_bert_embed(ids, ids_stride, nullptr, offs, lens, B, T, rows, word, pos, pos_offset, gamma, beta, out_f16, d, vocab, eps,
                            (hipStream_t)stream));
  return CLIPX_OK;
}

extern "C" int clipx_postln_f16_device(int device, void* x16, const float* gamma, const float* beta, int M, int d, float eps, void* stream) {
  if (!x16 || !gamma || !beta || M <= 0) return bfail(CLIPX_E_ARG, "bad postln arguments");
  int r = bert_check_d(d);
  if (r) return r;
  BHIPCHK(hipSetDevice(device));
  BHIPCHK(launch_postln_f16(x16, gamma, beta, M, d, eps, nullptr, (hipStream_t)stream));
  return CLIPX_OK;
}

extern "C" int clipx_bert_pool_device(int device, const void* x16, const int32_t* offs, const int32_t* lens, const float* W, const float* bias,
                                      float* y_raw, float* out_f32, uint16_t* out_f16, int B, int d, int E, void* stream) {
  if (!x16 || !offs || !lens || !W || !y_raw || !out_f32 || B <= 0 || E <= 0) return bfail(CLIPX_E_ARG, "bad bert_pool arguments");
  if (d <= 0 || d % 32 || d > 2048) return bfail(CLIPX_E_UNSUPPORTED, "d must be a multiple of 32, <= 2048");
  BHIPCHK(hipSetDevice(device));
  BHIPCHK(launch_bert_pool(x16, offs, lens, W, bias, y_raw, out_f32, out_f16, B, d, E, (hipStream_t)stream));
  return CLIPX_OK;
}
