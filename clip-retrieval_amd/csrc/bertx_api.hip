// bertx_api.hip -- host side of the clipx_bert_* part of include/clipx.h: the multilingual text towers of the reference's
// `use_mclip` (clip_inference/mapper.py:44-47, 62-63: SentenceTransformer(...).encode; clip_back.py:837-859: M-CLIP's XLM-R +
// LinearTransformation), one post-LN BERT-family encoder on the CLIP encoder's GEMMs and ragged attention plus the three kernels
// of bert_kernels.hip.  A batch is always ragged: sample b owns lens[b] packed rows, padded to whole 256-row GEMM tiles with
// pseudo-samples by the planner the CLIP text tower uses (clipx_ragged_plan.h).  No hipGraphs, no CPU compute path.

#include "bert_kernels.h"
#include "clipx_host.h"

using namespace clipx;

namespace {

constexpr int BERT_MAX_LEN = 128;   // the ragged attention kernels: head dimension 64, at most 128 tokens

struct BertLayer {
  const float *qkv_b, *out_b, *ln_att_w, *ln_att_b, *fc1_b, *fc2_b, *ln_out_w, *ln_out_b;  // into the f32 device blob
  bf16 *qkv_w, *fc1_w;  // IEEE fp16 bits behind the bf16-typed pointer: the GEMMs whose A operand is the fp16 stream
  bf16 *out_w, *fc2_w;  // bf16: the GEMMs whose A operand is the attention output / the GELU output
};

struct BertWeights : Weights {
  const float *word = nullptr, *pos = nullptr, *ln_emb_w = nullptr, *ln_emb_b = nullptr, *dense_w = nullptr, *dense_b = nullptr;
  std::vector<BertLayer> L;
};

// activation workspace, and the device side of what a host-pointer call's results travel back through
struct BertWorkspace {
  DevBuf<bf16> x, qkv, att, hbuf;  // x = the residual stream, IEEE fp16 [rows, width]
  DevBuf<float> ones;              // [rows] row scales of the fp16-operand GEMMs (no LayerNorm is folded into them here)
  DevBuf<float> y_raw;             // [max_batch, out_dim] the dense layer's output in front of the norm
  DevBuf<float> out32;             // host-pointer calls: the chunk's results on their way back
  DevBuf<uint16_t> out16;
  hipError_t alloc(size_t Bm, const clipx_bert_desc& d, hipStream_t st) {
    const size_t rows = ragged_max_rows(Bm, d.max_len), w = d.width, BE = Bm * d.out_dim;
    hipError_t e = hipSuccess;
    dev_alloc(e, x, rows * w);
    dev_alloc(e, qkv, rows * 3 * w);
    dev_alloc(e, att, rows * w);
    dev_alloc(e, hbuf, rows * d.mlp);
    dev_alloc(e, ones, rows);
    if (e == hipSuccess) e = launch_fill_f32(ones, 1.f, (int64_t)rows, st);
    dev_alloc(e, y_raw, BE);
    dev_alloc(e, out32, BE);
    dev_alloc(e, out16, BE);
    if (e != hipSuccess) *this = BertWorkspace();
    return e;
  }
};

}  // namespace

#pragma GCC visibility push(hidden)  // (the handle is no part of the ABI, only the pointer to it)
struct clipx_bert {
  clipx_bert_desc desc{};
  int device = 0;
  int max_batch = 256;
  int n_cu = 256;
  std::mutex mu;
  // (destroyed bottom-up: the stream is declared first, so that every buffer and event below goes before it)
  Stream stream;
  BertWeights w;
  BertWorkspace ws;
  PinBuf out_host;  // page-locked: f32 [max_batch, E] then f16 [max_batch, E]
  WsGate gate;  // its calls are never captured (they always upload per-call host data): the gate's capture check never fires
  // Per chunk: lens / offs / src of its samples and pseudo-samples (clipx_ragged_plan.h) and, behind them for host callers, the ids
  IntRing ring;
  size_t ids_at = 0;  // where in a slot the ids start
  RangeGuard range;   // one flag, raised by postln_f16_kernel
};
#pragma GCC visibility pop

extern "C" size_t clipx_bert_blob_floats(const clipx_bert_desc* d) {
  if (!d) return 0;
  const size_t w = d->width, mlp = d->mlp, E = d->out_dim;
  const size_t layer = 3 * w * w + 3 * w + w * w + w + 2 * w + mlp * w + mlp + w * mlp + w + 2 * w;
  return (size_t)d->vocab * w + (size_t)d->max_pos * w + 2 * w + (size_t)d->layers * layer + E * w + (d->dense_bias ? E : 0);
}

static int bert_check_desc(const clipx_bert_desc* d) {
  if (d->width <= 0 || d->width % 128 || d->width > 2048) return fail(CLIPX_E_UNSUPPORTED, "width must be a multiple of 128, at most 2048");
  if (d->heads <= 0 || d->width % d->heads) return fail(CLIPX_E_ARG, "width must be a multiple of heads");
  if (d->width / d->heads != 64) return fail(CLIPX_E_UNSUPPORTED, "the ragged attention kernels of this build need head dimension 64");
  if (d->max_len > BERT_MAX_LEN) return fail(CLIPX_E_UNSUPPORTED, "texts of more than 128 tokens have no ragged attention kernel");
  if (d->mlp <= 0 || d->mlp % 128) return fail(CLIPX_E_UNSUPPORTED, "mlp width must be a multiple of 128");
  if (d->max_len < 1 || d->layers <= 0 || d->vocab <= 0 || d->out_dim <= 0) return fail(CLIPX_E_ARG, "bad layer / vocab / length / out_dim");
  if (d->pos_offset < 0 || d->pos_offset + d->max_len > d->max_pos) return fail(CLIPX_E_ARG, "pos_offset + max_len exceeds the position table");
  if (!(d->ln_eps > 0.f)) return fail(CLIPX_E_ARG, "ln_eps must be positive");
  return 0;
}

static int bert_create_impl(clipx_bert* h, const float* blob, size_t blob_floats) {
  const clipx_bert_desc& d = h->desc;
  const size_t w = d.width, mlp = d.mlp, E = d.out_dim;
  BertWeights& W = h->w;
  HIPCHK(h->stream.create());
  hipStream_t st = h->stream;
  HIPCHK(W.upload(blob, blob_floats));
  float* p = W.blob;
  W.word = p; p += (size_t)d.vocab * w;
  W.pos = p; p += (size_t)d.max_pos * w;
  W.ln_emb_w = p; p += w;
  W.ln_emb_b = p; p += w;
  W.L.resize(d.layers);
  for (int l = 0; l < d.layers; ++l) {
    BertLayer& L = W.L[l];
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
    HIPCHK(W.take(&L.qkv_w, 3 * w * w));
    HIPCHK(W.take(&L.out_w, w * w));
    HIPCHK(W.take(&L.fc1_w, mlp * w));
    HIPCHK(W.take(&L.fc2_w, w * mlp));
    // the existing GEMMs take fp16 x fp16 (A = the fp16 stream) and bf16 x bf16: the weights are converted once, here
    HIPCHK(launch_f32_to_f16(qkv32, L.qkv_w, (int64_t)(3 * w * w), st));
    HIPCHK(launch_f32_to_bf16(out32, L.out_w, (int64_t)(w * w), st));
    HIPCHK(launch_f32_to_f16(fc1_32, L.fc1_w, (int64_t)(mlp * w), st));
    HIPCHK(launch_f32_to_bf16(fc2_32, L.fc2_w, (int64_t)(w * mlp), st));
  }
  W.dense_w = p; p += E * w;
  if (d.dense_bias) { W.dense_b = p; p += E; }
  if ((size_t)(p - W.blob.p) != blob_floats) return fail(CLIPX_E_ARG, "internal: blob carve does not match clipx_bert_blob_floats");

  const size_t Bm = h->max_batch;
  HIPCHK(h->ws.alloc(Bm, d, st));
  HIPCHK(h->out_host.ensure(Bm * E * (sizeof(float) + sizeof(uint16_t))));
  h->ids_at = ragged_slot_ints(Bm, d.max_len, false);
  HIPCHK(h->ring.alloc(h->ids_at + Bm * d.max_len));
  HIPCHK(h->range.alloc(1, st));
  HIPCHK(h->gate.alloc());
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int clipx_bert_create(const clipx_bert_desc* desc, const float* blob, size_t blob_floats, int device, clipx_bert** out) {
  if (!desc || !blob || !out) return fail(CLIPX_E_ARG, "null argument");
  *out = nullptr;
  int r = bert_check_desc(desc), n_cu = 0;
  if (r) return r;
  if (blob_floats != clipx_bert_blob_floats(desc)) return fail(CLIPX_E_ARG, "weight blob has the wrong number of floats for this model description");
  if ((r = open_device(device, &n_cu))) return r;
  clipx_bert* h = new clipx_bert();
  h->desc = *desc;
  h->device = device;
  h->n_cu = n_cu;
  h->max_batch = env_positive("CLIPX_MAX_BATCH", h->max_batch);
  if ((r = bert_create_impl(h, blob, blob_floats))) {
    clipx_bert_destroy(h);  // (sets no message: g_err keeps what failed)
    return r;
  }
  *out = h;
  return CLIPX_OK;
}

extern "C" void clipx_bert_destroy(clipx_bert* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
}

extern "C" int clipx_bert_out_dim(const clipx_bert* h) { return h ? h->desc.out_dim : 0; }

static int bert_gemm(clipx_bert* h, hipStream_t st, const bf16* A, const bf16* W, const float* bias, void* out, int M, int N, int K, int epi,
                     bool f16) {
  GemmArgs g{};
  g.A = A; g.W = W; g.bias = bias; g.out = out; g.T = 1;
  g.M = M; g.N = N; g.K = K; g.epi = epi; g.variant = clipx::GEMM_V_DEFAULT; g.n_cu = h->n_cu;
  g.rowscale = f16 ? h->ws.ones.p : nullptr;
  g.f16 = f16 ? 1 : 0;
  HIPCHK(launch_gemm(g, st));
  return 0;
}

// One chunk (nb <= max_batch samples whose lengths were checked), everything on the device, asynchronous on `st`.  ids_dev: int32
// [nb, max_len].  Slot `s` of the ring is the caller's (IntRing::take); its event is recorded here, behind the upload of the description.
static int bert_chunk(clipx_bert* h, hipStream_t st, int s, const int32_t* ids_dev, const int32_t* lens_host, int nb, float* out32,
                      uint16_t* out16) {
  const clipx_bert_desc& d = h->desc;
  const BertWeights& W = h->w;
  const BertWorkspace& ws = h->ws;
  const int w = d.width;
  int M = 0;
  for (int b = 0; b < nb; ++b) M += lens_host[b];
  const int Mp = gemm256_whole_tile_rows(M, 3 * w, w, clipx::GEMM_V_DEFAULT, h->n_cu);
  int* slot = h->ring.ints(s);
  const RaggedPlan p = ragged_complete(slot, lens_host, nb, d.max_len, Mp, false);
  if (!p.S) return fail(CLIPX_E_ARG, "internal: the activation workspace does not hold the padded rows");
  int r = h->ring.upload(s, p.ints, st);
  if (r) return r;
  const int* dev = h->ring.dev[s];
  const int *src_d = dev + (p.src - slot), *lens_d = dev + (p.lens - slot), *offs_d = dev + (p.offs - slot);
  const int S = p.S, lmax = p.lmax;
  int* flag = h->range.flag(0);

  HIPCHK(launch_bert_embed(ids_dev, d.max_len, src_d, offs_d, lens_d, S, lmax, Mp, W.word, W.pos, d.pos_offset, W.ln_emb_w, W.ln_emb_b,
                            ws.x, w, d.vocab, d.ln_eps, st));
  // Per layer (post-LN: each LayerNorm rewrites the stream, it is both the next GEMM's operand and the next residual):
  //   qkv = fp16(x Wqkv^T + b)                     fp16 MFMA, epilogue 7
  //   att = attention(qkv), not causal, keys of the sample's own rows only
  //   x = fp16(x + att Wout^T + b); x = LN_att(x)  bf16 MFMA, epilogue 6 (f32 add), then postln in place
  //   h = bf16(gelu(x Wfc1^T + b))                 fp16 MFMA, epilogue 2
  //   x = fp16(x + h Wfc2^T + b); x = LN_out(x)    bf16 MFMA, epilogue 6, postln
  for (int l = 0; l < d.layers; ++l) {
    const BertLayer& L = W.L[l];
    if ((r = bert_gemm(h, st, ws.x, L.qkv_w, L.qkv_b, ws.qkv, Mp, 3 * w, w, EPI_BIAS_F16, true))) return r;
    HIPCHK(launch_attention(ws.qkv, ws.att, S, lmax, d.heads, 64, 0, st, 0, offs_d, lens_d));
    if ((r = bert_gemm(h, st, ws.att, L.out_w, L.out_b, ws.x, Mp, w, w, EPI_BIAS_RESID_H16, false))) return r;
    HIPCHK(launch_postln_f16(ws.x, L.ln_att_w, L.ln_att_b, Mp, w, d.ln_eps, flag, st));
    if ((r = bert_gemm(h, st, ws.x, L.fc1_w, L.fc1_b, ws.hbuf, Mp, d.mlp, w, EPI_BIAS_GELU_BF16, true))) return r;
    if ((r = bert_gemm(h, st, ws.hbuf, L.fc2_w, L.fc2_b, ws.x, Mp, w, d.mlp, EPI_BIAS_RESID_H16, false))) return r;
    HIPCHK(launch_postln_f16(ws.x, L.ln_out_w, L.ln_out_b, Mp, w, d.ln_eps, flag, st));
  }
  HIPCHK(launch_bert_pool(ws.x, offs_d, lens_d, W.dense_w, W.dense_b, ws.y_raw, out32, out16, nb, w, d.out_dim, st));
  return 0;
}

static int bert_check_lens(const clipx_bert* h, const int32_t* lens, int B) {
  for (int b = 0; b < B; ++b)
    if (lens[b] < 1 || lens[b] > h->desc.max_len)
      return fail(CLIPX_E_ARG, "lens[" + std::to_string(b) + "] = " + std::to_string(lens[b]) + " is outside 1 .. max_len = " +
                                    std::to_string(h->desc.max_len));
  return 0;
}

extern "C" int clipx_bert_encode(clipx_bert* h, const int32_t* ids, const int32_t* lens, int B, float* out_f32, uint16_t* out_f16) {
  if (!h || !ids || !lens || !out_f32 || B < 1) return fail(CLIPX_E_ARG, "bad bert_encode arguments");
  int r = bert_check_lens(h, lens, B);
  if (r) return r;
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  const clipx_bert_desc& d = h->desc;
  const size_t E = d.out_dim;
  hipStream_t st = h->stream;
  if ((r = h->gate.acquire(st))) return r;
  bool overflow = false;
  for (int o = 0; o < B; o += h->max_batch) {
    const int nb = std::min(h->max_batch, B - o);
    int s;
    if ((r = h->ring.take(&s))) return r;
    int* ids_pin = h->ring.ints(s) + h->ids_at;
    int* ids_dev = h->ring.dev[s] + h->ids_at;
    // rows are copied whole; positions past lens[b] are never read on the device (the embedding kernel's mask)
    memcpy(ids_pin, ids + (size_t)o * d.max_len, (size_t)nb * d.max_len * sizeof(int32_t));
    HIPCHK(hipMemcpyAsync(ids_dev, ids_pin, (size_t)nb * d.max_len * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((r = bert_chunk(h, st, s, ids_dev, lens + o, nb, h->ws.out32, out_f16 ? h->ws.out16.p : nullptr))) return r;
    char* po = (char*)h->out_host.p;
    HIPCHK(hipMemcpyAsync(po, h->ws.out32, (size_t)nb * E * sizeof(float), hipMemcpyDeviceToHost, st));
    if (out_f16) HIPCHK(hipMemcpyAsync(po + (size_t)h->max_batch * E * sizeof(float), h->ws.out16, (size_t)nb * E * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    if ((r = h->range.read_back(0, st))) return r;
    HIPCHK(hipStreamSynchronize(st));
    memcpy(out_f32 + (size_t)o * E, po, (size_t)nb * E * sizeof(float));
    if (out_f16) memcpy(out_f16 + (size_t)o * E, po + (size_t)h->max_batch * E * sizeof(float), (size_t)nb * E * sizeof(uint16_t));
    if (h->range.test_and_clear(0)) overflow = true;
  }
  if ((r = h->gate.release(st))) return r;
  return overflow ? RangeGuard::overflow() : CLIPX_OK;
}

extern "C" int clipx_bert_encode_device(clipx_bert* h, const int32_t* ids_dev, const int32_t* lens_host, int B, float* out_f32_dev,
                                        uint16_t* out_f16_dev, void* stream) {
  if (!h || !ids_dev || !lens_host || !out_f32_dev || B < 1) return fail(CLIPX_E_ARG, "bad bert_encode_device arguments");
  int r = bert_check_lens(h, lens_host, B);
  if (r) return r;
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  const clipx_bert_desc& d = h->desc;
  const size_t E = d.out_dim;
  hipStream_t st = stream ? (hipStream_t)stream : h->stream.s;
  if ((r = h->gate.acquire(st))) return r;
  for (int o = 0; o < B; o += h->max_batch) {
    const int nb = std::min(h->max_batch, B - o);
    int s;
    if ((r = h->ring.take(&s))) return r;
    if ((r = bert_chunk(h, st, s, ids_dev + (size_t)o * d.max_len, lens_host + o, nb, out_f32_dev + (size_t)o * E,
                        out_f16_dev ? out_f16_dev + (size_t)o * E : nullptr)))
      return r;
  }
  return h->gate.release(st);
}

extern "C" int clipx_bert_range_check(clipx_bert* h, void* stream) {
  if (!h) return fail(CLIPX_E_ARG, "handle is null");
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  return h->range.check(0, stream ? (hipStream_t)stream : h->stream.s);
}

// ---------------------------------------------------------------------------------------------
// the three kernels in isolation (per-kernel parity tests)
// ---------------------------------------------------------------------------------------------
static int bert_check_d(int d) {
  if (d <= 0 || d % 128 || d > 2048) return fail(CLIPX_E_UNSUPPORTED, "d must be a multiple of 128, <= 2048");
  return 0;
}

extern "C" int clipx_bert_embed_device(int device, const int32_t* ids, int ids_stride, const int32_t* offs, const int32_t* lens, int B, int T,
                                       int rows, const float* word, const float* pos, int pos_offset, int max_pos, const float* gamma,
                                       const float* beta, void* out_f16, int d, int vocab, float eps, void* stream) {
  if (!ids || !offs || !lens || !word || !pos || !gamma || !beta || !out_f16 || B <= 0 || rows <= 0 || vocab <= 0)
    return fail(CLIPX_E_ARG, "bad bert_embed arguments");
  if (T < 1 || pos_offset < 0 || pos_offset + T > max_pos) return fail(CLIPX_E_ARG, "positions pos_offset .. pos_offset + T - 1 must lie inside the position table");
  if (ids_stride < 0 || (ids_stride > 0 && ids_stride < T)) return fail(CLIPX_E_ARG, "ids_stride must be 0 (packed ids) or at least T");
  int r = bert_check_d(d);
  if (r) return r;
  HIPCHK(hipSetDevice(device));
  HIPCHK(launch_bert_embed(ids, ids_stride, nullptr, offs, lens, B, T, rows, word, pos, pos_offset, gamma, beta, out_f16, d, vocab, eps,
                            (hipStream_t)stream));
  return CLIPX_OK;
}

extern "C" int clipx_postln_f16_device(int device, void* x16, const float* gamma, const float* beta, int M, int d, float eps, void* stream) {
  if (!x16 || !gamma || !beta || M <= 0) return fail(CLIPX_E_ARG, "bad postln arguments");
  int r = bert_check_d(d);
  if (r) return r;
  HIPCHK(hipSetDevice(device));
  HIPCHK(launch_postln_f16(x16, gamma, beta, M, d, eps, nullptr, (hipStream_t)stream));
  return CLIPX_OK;
}

extern "C" int clipx_bert_pool_device(int device, const void* x16, const int32_t* offs, const int32_t* lens, const float* W, const float* bias,
                                      float* y_raw, float* out_f32, uint16_t* out_f16, int B, int d, int E, void* stream) {
  if (!x16 || !offs || !lens || !W || !y_raw || !out_f32 || B <= 0 || E <= 0) return fail(CLIPX_E_ARG, "bad bert_pool arguments");
  if (d <= 0 || d % 32 || d > 2048) return fail(CLIPX_E_UNSUPPORTED, "d must be a multiple of 32, <= 2048");
  HIPCHK(hipSetDevice(device));
  HIPCHK(launch_bert_pool(x16, offs, lens, W, bias, y_raw, out_f32, out_f16, B, d, E, (hipStream_t)stream));
  return CLIPX_OK;
}
