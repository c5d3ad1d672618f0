// clipx_api.hip -- host side of the C ABI declared in include/clipx.h (encode half of the hot path): the model description, the
// weight blob, create / destroy, options and getters, and the entry points that take device buffers.
//
// Stands in for `model.encode_image` / `model.encode_text` + normalise + fp16 as called by
// ClipMapper.__call__ (reference clip_retrieval/clip_inference/mapper.py:49-78).  Owns the bf16/f32
// weights in HBM, one activation workspace sized for `max_batch`, a compute stream, a copy stream
// and pinned staging slots (H2D of chunk n+1 overlaps the kernels of chunk n: clipx_host_path.hip).
// There is deliberately no CPU compute path: without a gfx950 device every entry point fails.

#include "clipx_attn_plan.h"
#include "clipx_host.h"

using namespace clipx;

extern "C" const char* clipx_last_error(void) { return g_err.c_str(); }

extern "C" size_t clipx_blob_floats(const clipx_model_desc* d) {
  if (!d) return 0;
  auto layer = [](size_t w, size_t mlp) {
    return 2 * w + 3 * w * w + 3 * w + w * w + w + 2 * w + mlp * w + mlp + w * mlp + w;
  };
  const size_t g = d->image_size / d->patch_size, Tv = g * g + 1;
  const size_t w = d->v_width, tw = d->t_width, E = d->embed_dim;
  size_t n = w * 3 * d->patch_size * d->patch_size + w + Tv * w + 2 * w;
  n += (size_t)d->v_layers * layer(w, d->v_mlp) + 2 * w + E * w;
  n += (size_t)d->vocab * tw + (size_t)d->ctx_len * tw;
  n += (size_t)d->t_layers * layer(tw, d->t_mlp) + 2 * tw + E * tw;
  return n;
}

static int check_desc(const clipx_model_desc* d) {
  if (d->image_size <= 0 || d->patch_size <= 0 || d->image_size % d->patch_size) return fail(CLIPX_E_ARG, "image_size must be a multiple of patch_size");
  if (d->v_width % 128 || d->t_width % 128 || d->v_width > 2048 || d->t_width > 2048)
    return fail(CLIPX_E_UNSUPPORTED, "tower widths must be multiples of 128, at most 2048");
  if (d->v_width % d->v_heads || d->t_width % d->t_heads) return fail(CLIPX_E_ARG, "width must be a multiple of heads");
  const int vdh = d->v_width / d->v_heads, tdh = d->t_width / d->t_heads;
  if (tdh != 64 && tdh != 80) return fail(CLIPX_E_UNSUPPORTED, "this build has text-tower attention kernels for head dimensions 64 and 80 only");
  if (vdh != 64 && vdh != 80 && !clipx::attn_wide_head(vdh))
    return fail(CLIPX_E_UNSUPPORTED, "this build has image-tower attention kernels for head dimensions 64, 80, 88 and 104 only");
  if (d->v_mlp % 128 || d->t_mlp % 128) return fail(CLIPX_E_UNSUPPORTED, "mlp widths must be multiples of 128");
  const int g = d->image_size / d->patch_size;
  // the image tower may be long where the long-sequence attention kernel exists (head dimension 64, not causal: clipx_attn_plan.h)
  if (d->ctx_len > clipx::ATTN_SHORT_MAX_T) return fail(CLIPX_E_UNSUPPORTED, "text context longer than 288 tokens");
  // (head dimension 80 at 97 .. 256 tokens has no kernel either, and is left to fail at its first launch as it always has)
  if (g * g + 1 > clipx::ATTN_LONG_MAX_T) return fail(CLIPX_E_UNSUPPORTED, "image sequence longer than 608 tokens");
  if (g * g + 1 > clipx::ATTN_SHORT_MAX_T && vdh != 64)
    return fail(CLIPX_E_UNSUPPORTED, "image sequence longer than 288 tokens at a head dimension other than 64");
  // head dimensions 88 and 104 (ViT-g/14, ViT-bigG/14) have the key-block counts 1 .. 3 and 9 only: refused here, not at the first launch
  if (clipx::attn_wide_head(vdh) && clipx::attn_plan(g * g + 1, vdh, 0).kernel == clipx::ATTN_NONE)
    return fail(CLIPX_E_UNSUPPORTED, "image-tower head dimensions 88 and 104 need at most 96 image tokens, or 257 .. 288");
  if (d->embed_dim <= 0 || d->embed_dim % 8) return fail(CLIPX_E_ARG, "embed_dim must be a multiple of 8");
  if (d->act != CLIPX_ACT_QUICK_GELU && d->act != CLIPX_ACT_GELU) return fail(CLIPX_E_ARG, "unknown activation");
  if (d->v_layers <= 0 || d->t_layers <= 0 || d->vocab <= 0 || d->ctx_len <= 0) return fail(CLIPX_E_ARG, "bad layer/vocab/context size");
  return 0;
}

// carve one transformer tower's per-layer parameters out of the device blob, converting matrices to bf16
static int carve_layers(ClipWeights& W, hipStream_t st, Tower& t, float*& p) {
  const size_t w = t.width, mlp = t.mlp;
  t.L.resize(t.layers);
  for (int l = 0; l < t.layers; ++l) {
    LayerW& L = t.L[l];
    L.ln1_w = p; p += w;
    L.ln1_b = p; p += w;
    const float* qkv_w32 = p; p += 3 * w * w;
    L.qkv_b = p; p += 3 * w;
    const float* out_w32 = p; p += w * w;
    L.out_b = p; p += w;
    L.ln2_w = p; p += w;
    L.ln2_b = p; p += w;
    const float* fc1_w32 = p; p += mlp * w;
    L.fc1_b = p; p += mlp;
    const float* fc2_w32 = p; p += w * mlp;
    L.fc2_b = p; p += w;
    HIPCHK(W.take(&L.qkv_w, 3 * w * w));
    HIPCHK(W.take(&L.out_w, w * w));
    HIPCHK(W.take(&L.fc1_w, mlp * w));
    HIPCHK(W.take(&L.fc2_w, w * mlp));
    HIPCHK(W.take(&L.qkv_c, 3 * w));
    HIPCHK(W.take(&L.fc1_c, mlp));
    HIPCHK(launch_fold_layernorm(qkv_w32, L.ln1_w, L.ln1_b, L.qkv_b, L.qkv_w, L.qkv_c, (int)(3 * w), (int)w, st, 1));
    HIPCHK(launch_f32_to_bf16(out_w32, L.out_w, (int64_t)(w * w), st));
    HIPCHK(launch_fold_layernorm(fc1_w32, L.ln2_w, L.ln2_b, L.fc1_b, L.fc1_w, L.fc1_c, (int)mlp, (int)w, st, 1));
    HIPCHK(launch_f32_to_bf16(fc2_w32, L.fc2_w, (int64_t)(w * mlp), st));
  }
  return 0;
}

static int create_impl(clipx_handle* h, const float* blob, size_t blob_floats) {
  const clipx_model_desc& d = h->desc;
  const int g = d.image_size / d.patch_size;
  ClipWeights& W = h->w;
  Tower& V = W.vis;
  Tower& X = W.txt;
  V.width = d.v_width; V.layers = d.v_layers; V.heads = d.v_heads; V.mlp = d.v_mlp; V.T = g * g + 1;
  X.width = d.t_width; X.layers = d.t_layers; X.heads = d.t_heads; X.mlp = d.t_mlp; X.T = d.ctx_len;
  W.PP3 = 3 * d.patch_size * d.patch_size;
  W.Kp = (W.PP3 + 63) / 64 * 64;
  const size_t E = d.embed_dim;

  HIPCHK(h->stream.create());
  HIPCHK(h->copy_stream.create());
  HIPCHK(W.upload(blob, blob_floats));

  int r;
  float* p = W.blob;
  // ---- vision
  const float* conv32 = p; p += (size_t)V.width * W.PP3;
  const float* cls = p; p += V.width;
  const float* vpos = p; p += (size_t)V.T * V.width;
  W.ln_pre_w = p; p += V.width;
  W.ln_pre_b = p; p += V.width;
  HIPCHK(W.take(&W.conv_w, (size_t)V.width * W.Kp));
  HIPCHK(launch_pad_rows_bf16(conv32, W.conv_w, V.width, W.PP3, W.Kp, h->stream));
  HIPCHK(W.take(&W.clspos, (size_t)V.T * V.width));
  HIPCHK(hipMemcpyAsync(W.clspos, vpos, (size_t)V.T * V.width * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  {  // row 0 += class embedding (host arithmetic on a tiny row, then upload)
    const size_t off_cls = (size_t)(cls - W.blob.p), off_pos = (size_t)(vpos - W.blob.p);
    std::vector<float> row0(V.width);
    for (int i = 0; i < V.width; ++i) row0[i] = blob[off_cls + i] + blob[off_pos + i];
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(W.clspos, row0.data(), V.width * sizeof(float), hipMemcpyHostToDevice));
  }
  if ((r = carve_layers(W, h->stream, V, p))) return r;
  V.lnf_w = p; p += V.width;
  V.lnf_b = p; p += V.width;
  const float* vproj32 = p; p += E * V.width;
  HIPCHK(W.take(&V.proj, E * V.width));
  HIPCHK(launch_f32_to_bf16(vproj32, V.proj, (int64_t)(E * V.width), h->stream));
  // ---- text
  W.tok_emb = p; p += (size_t)d.vocab * X.width;
  W.txt_pos = p; p += (size_t)X.T * X.width;
  if ((r = carve_layers(W, h->stream, X, p))) return r;
  X.lnf_w = p; p += X.width;
  X.lnf_b = p; p += X.width;
  const float* tproj32 = p; p += E * X.width;
  HIPCHK(W.take(&X.proj, E * X.width));
  HIPCHK(launch_f32_to_bf16(tproj32, X.proj, (int64_t)(E * X.width), h->stream));
  if ((size_t)(p - W.blob.p) != blob_floats) return fail(CLIPX_E_ARG, "internal: blob carve does not match clipx_blob_floats");

  const size_t Bm = h->max_batch;
  HIPCHK(h->ws.alloc(Bm, V, X, W.Kp));
  HIPCHK(h->gate.alloc());
  HIPCHK(h->slots.alloc(std::max(Bm * pix_bytes_per_image(d, CLIPX_PIX_F32_NCHW), Bm * d.ctx_len * sizeof(int32_t)), Bm * E));
  HIPCHK(h->range.alloc(StagingSlots::N + 1, h->stream));
  HIPCHK(h->ragged.alloc(ragged_slot_ints(Bm, X.T, true)));
  HIPCHK(h->ids_back.ensure(Bm * X.T * sizeof(int32_t)));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int clipx_create(const clipx_model_desc* desc, const float* blob, size_t blob_floats, int device,
                            clipx_handle** out) {
  if (!desc || !blob || !out) return fail(CLIPX_E_ARG, "null argument");
  *out = nullptr;
  int r = check_desc(desc), n_cu = 0;
  if (r) return r;
  if (blob_floats != clipx_blob_floats(desc)) return fail(CLIPX_E_ARG, "weight blob has the wrong number of floats for this model description");
  if ((r = open_device(device, &n_cu))) return r;
  clipx_handle* h = new clipx_handle();
  h->desc = *desc;
  h->device = device;
  h->n_cu = n_cu;
  h->max_batch = env_positive("CLIPX_MAX_BATCH", h->max_batch);
  h->host_chunk = std::min(env_positive("CLIPX_HOST_CHUNK", h->host_chunk), h->max_batch);
  const char* gv = getenv("CLIPX_GEMM_VARIANT");
  if (gv) h->gemm_variant = std::min((int)clipx::GEMM_V_MAX, std::max(0, atoi(gv)));  // 5: tools build only (falls back to 3 in the product)
  const char* lf = getenv("CLIPX_LN_FUSED");
  if (lf) h->ln_fused = lf[0] == '1';
  const char* rgt = getenv("CLIPX_RAGGED_TEXT");
  if (rgt && rgt[0] == '0') h->ragged_text = false;
  const char* fl = getenv("CLIPX_FULL_LAST_BLOCK");
  if (fl && atoi(fl) > 0) h->pool_last_block = false;
  if ((r = create_impl(h, blob, blob_floats))) {
    clipx_destroy(h);  // (sets no message: g_err keeps what failed)
    return r;
  }
  *out = h;
  return CLIPX_OK;
}

extern "C" void clipx_destroy(clipx_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
  delete h;
}

extern "C" int clipx_set_option(clipx_handle* h, int option, int value) {
  if (!h) return fail(CLIPX_E_ARG, "handle is null");
  std::lock_guard<std::mutex> lk(h->mu);
  switch (option) {
    case CLIPX_OPT_RAGGED_TEXT: h->ragged_text = value != 0; return CLIPX_OK;
    case CLIPX_OPT_POOL_LAST_BLOCK: h->pool_last_block = value != 0; return CLIPX_OK;
    case CLIPX_OPT_PROF_MARKERS: h->prof.markers = value != 0; return CLIPX_OK;
    default: return fail(CLIPX_E_ARG, "unknown option");
  }
}
extern "C" int clipx_get_option(const clipx_handle* h, int option) {
  if (!h) return -1;
  switch (option) {
    case CLIPX_OPT_RAGGED_TEXT: return h->ragged_text ? 1 : 0;
    case CLIPX_OPT_POOL_LAST_BLOCK: return h->pool_last_block ? 1 : 0;
    case CLIPX_OPT_PROF_MARKERS: return h->prof.markers ? 1 : 0;
    default: return -1;
  }
}
extern "C" int clipx_max_batch(const clipx_handle* h) { return h ? h->max_batch : 0; }
extern "C" int clipx_graphs_cached(const clipx_handle* h) { return h ? (int)h->graphs.execs.size() : 0; }
extern "C" int clipx_last_text_rows(const clipx_handle* h) { return h ? h->last_text_rows : 0; }
extern "C" int clipx_embed_dim(const clipx_handle* h) { return h ? h->desc.embed_dim : 0; }

// ---------------------------------------------------------------------------------------------
// device buffers in, device buffers out, asynchronous on the caller's stream (or the handle's)
// ---------------------------------------------------------------------------------------------
extern "C" int clipx_encode_image_device(clipx_handle* h, const void* pixels_dev, int B, int pix_fmt, uint16_t* out_f16_dev,
                                         float* out_f32_or_null, void* stream) {
  if (!h || !pixels_dev || !out_f16_dev || B < 0) return fail(CLIPX_E_ARG, "bad encode_image arguments");
  if (pix_fmt != CLIPX_PIX_F32_NCHW && pix_fmt != CLIPX_PIX_U8_NHWC) return fail(CLIPX_E_ARG, "unknown pixel format");
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  const Call c{stream ? (hipStream_t)stream : h->stream.s, B == 1, h->range.flag(StagingSlots::N), nullptr};
  const size_t ib = pix_bytes_per_image(h->desc, pix_fmt), E = h->desc.embed_dim;
  if (h->gate.acquire(c.st)) return CLIPX_E_HIP;
  for (int o = 0; o < B; o += h->max_batch) {
    const int nb = std::min(h->max_batch, B - o);
    int r = vision_chunk(h, c, (const char*)pixels_dev + (size_t)o * ib, nb, pix_fmt, out_f16_dev + (size_t)o * E,
                         out_f32_or_null ? out_f32_or_null + (size_t)o * E : nullptr);
    if (r) return r;
  }
  if (h->gate.release(c.st)) return CLIPX_E_HIP;
  return CLIPX_OK;
}

static int encode_text_device_impl(clipx_handle* h, const int32_t* ids_dev, const int32_t* ids_host_or_null, int B, uint16_t* out_f16_dev,
                                   float* out_f32_or_null, void* stream) {
  if (!h || !ids_dev || !out_f16_dev || B < 0) return fail(CLIPX_E_ARG, "bad encode_text arguments");
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  Call c{stream ? (hipStream_t)stream : h->stream.s, B == 1, h->range.flag(StagingSlots::N), nullptr};
  const size_t E = h->desc.embed_dim, T = h->desc.ctx_len;
  if (h->gate.acquire(c.st)) return CLIPX_E_HIP;
  for (int o = 0; o < B; o += h->max_batch) {
    const int nb = std::min(h->max_batch, B - o);
    // the caller's host copy of the ids (the reader tokenised them there): the ragged row map is built without reading them back
    c.ids_host = ids_host_or_null ? ids_host_or_null + (size_t)o * T : nullptr;
    int r = text_chunk(h, c, ids_dev + (size_t)o * T, nb, out_f16_dev + (size_t)o * E,
                       out_f32_or_null ? out_f32_or_null + (size_t)o * E : nullptr);
    if (r) return r;
  }
  if (h->gate.release(c.st)) return CLIPX_E_HIP;
  return CLIPX_OK;
}

extern "C" int clipx_encode_text_device(clipx_handle* h, const int32_t* ids_dev, int B, uint16_t* out_f16_dev,
                                        float* out_f32_or_null, void* stream) {
  return encode_text_device_impl(h, ids_dev, nullptr, B, out_f16_dev, out_f32_or_null, stream);
}

extern "C" int clipx_encode_text_device_ids(clipx_handle* h, const int32_t* ids_dev, const int32_t* ids_host, int B, uint16_t* out_f16_dev,
                                            float* out_f32_or_null, void* stream) {
  if (!ids_host) return fail(CLIPX_E_ARG, "ids_host is null (use clipx_encode_text_device)");
  return encode_text_device_impl(h, ids_dev, ids_host, B, out_f16_dev, out_f32_or_null, stream);
}

extern "C" int clipx_range_check(clipx_handle* h, void* stream) {
  if (!h) return fail(CLIPX_E_ARG, "handle is null");
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  return h->range.check(StagingSlots::N, stream ? (hipStream_t)stream : h->stream.s);
}
