/*
 * clipx.h -- C ABI of the MI355X-native CLIP encoder (encode half of the hot path).
 *
 * This is the boundary a clip-retrieval maintainer binds (ctypes stub in INTEGRATION.md) to
 * replace the two model calls inside `ClipMapper.__call__`
 * (reference clip_retrieval/clip_inference/mapper.py:57 `self.model_img(...)`, :65
 * `self.model_txt(...)`) together with the normalise + fp16 cast that follows them
 * (mapper.py:58-59, 66-67), and the B=1 query encodes of `KnnService.compute_query`
 * (clip_back.py:230, 244).  Plain pointers and sizes only; no torch types.  Every function
 * returns 0 or a negative CLIPX_E_* code and never throws; clipx_last_error() is thread-local.
 *
 * Arithmetic: 16-bit MFMA operands (bf16; IEEE fp16 where the operand is the residual stream) with fp32 accumulation; the
 * residual stream is stored in fp16 and added to in fp32, LayerNorm statistics and softmax are fp32.  Outputs are unit-L2-norm
 * rows rounded to IEEE fp16, exactly the
 * `image_embs` / `text_embs` arrays the reference writer stores (writer.py:67-75).
 */
#ifndef CLIPX_H
#define CLIPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct clipx_handle clipx_handle;

enum {
  CLIPX_OK = 0,
  CLIPX_E_ARG = -1,
  CLIPX_E_HIP = -2,
  CLIPX_E_NOMEM = -3,
  CLIPX_E_STATE = -4,
  CLIPX_E_UNSUPPORTED = -5,
  CLIPX_E_RANGE = -6 /* the fp16 residual stream overflowed for these weights / inputs: the call's embeddings are invalid */
};

#define CLIPX_ACT_QUICK_GELU 0 /* OpenAI CLIP checkpoints (x * sigmoid(1.702 x)) */
#define CLIPX_ACT_GELU 1       /* open_clip LAION checkpoints (erf GELU)         */

#define CLIPX_PIX_F32_NCHW 0 /* f32 [B,3,S,S], already mean/std normalised: the reference's item["image_tensor"] */
#define CLIPX_PIX_U8_NHWC 1  /* u8  [B,S,S,3] raw RGB; /255, mean/std normalised on the device               */

/* Architecture of one CLIP model = what `all_clip.load_clip(clip_model)` resolves a name to
 * (mapper.py:36-41).  Tower widths are multiples of 128, at most 2048.  Head dimension (width / heads): 64 or 80 (ViT-H/14) for
 * either tower; the image tower also 88 (ViT-g/14: 1408 / 16) and 104 (ViT-bigG/14: 1664 / 16), there with at most 96 image tokens
 * or 257 .. 288 (224 pixels at patch 14 is 257).  CLIPX_E_UNSUPPORTED otherwise. */
typedef struct clipx_model_desc {
  int image_size;   /* 224 */
  int patch_size;   /* 14 (L/14), 32 (B/32), 16 (B/16) */
  int v_width;      /* 1024 */
  int v_layers;     /* 24 */
  int v_heads;      /* 16 */
  int v_mlp;        /* 4096 */
  int ctx_len;      /* 77 */
  int vocab;        /* 49408 */
  int t_width;      /* 768 */
  int t_layers;     /* 12 */
  int t_heads;      /* 12 */
  int t_mlp;        /* 3072 */
  int embed_dim;    /* 768 */
  int act;          /* CLIPX_ACT_* */
  float ln_eps;     /* 1e-5 */
  float pix_mean[3];/* CLIP mean (0.48145466, 0.4578275, 0.40821073) -- used by CLIPX_PIX_U8_NHWC */
  float pix_std[3]; /* CLIP std  (0.26862954, 0.26130258, 0.27577711) */
} clipx_model_desc;

/* Number of floats in the weight blob for `desc` (see the order below). */
size_t clipx_blob_floats(const clipx_model_desc* desc);

/* Create an encoder on HIP device `device` from a host f32 weight blob.  Blob order, all
 * row-major, torch `nn.Linear` [out, in] weights:
 *   vision:  conv1.weight [v_width, 3*P*P]; class_embedding [v_width]; positional_embedding [T_v, v_width];
 *            ln_pre.{w,b}; per layer { ln_1.{w,b}; in_proj_weight [3w, w] (q|k|v); in_proj_bias [3w];
 *            out_proj.{weight [w,w], bias}; ln_2.{w,b}; c_fc.{weight [mlp,w], bias}; c_proj.{weight [w,mlp], bias} };
 *            ln_post.{w,b}; visual projection [embed_dim, v_width]
 *   text:    token_embedding [vocab, t_width]; positional_embedding [ctx_len, t_width]; per layer (same as above);
 *            ln_final.{w,b}; text projection [embed_dim, t_width]
 * (T_v = (image_size/patch_size)^2 + 1).  The blob is consumed during the call. */
int clipx_create(const clipx_model_desc* desc, const float* blob, size_t blob_floats, int device,
                 clipx_handle** out);
void clipx_destroy(clipx_handle* h);

/* model.encode_image(x) + `/= norm` + `.to(float16)` (mapper.py:57-59).  pixels: host pointer,
 * layout per pix_fmt; out_f16: host [B, embed_dim] IEEE fp16 bits.  Any B >= 1 (chunked internally). */
int clipx_encode_image(clipx_handle* h, const void* pixels, int B, int pix_fmt, uint16_t* out_f16);

/* model.encode_text(tokens) + normalise + fp16 (mapper.py:65-67).  ids: host int32 [B, ctx_len]
 * (SOT ... EOT 0 0 ..; the pooled position is argmax(ids) like the reference model). */
int clipx_encode_text(clipx_handle* h, const int32_t* ids, int B, uint16_t* out_f16);

/* Same encoders with an f32 [B, embed_dim] result: the unit-norm embedding BEFORE the fp16 rounding.  The query side
 * (`KnnService.compute_query`, clip_back.py:230-232, 244-246) hands fp32 features to the index. */
int clipx_encode_image_f32(clipx_handle* h, const void* pixels, int B, int pix_fmt, float* out_f32);
int clipx_encode_text_f32(clipx_handle* h, const int32_t* ids, int B, float* out_f32);

/* Asynchronous tickets: the call stages the batch (B <= clipx_max_batch()), enqueues upload, kernels and
 * download, and returns; clipx_wait() blocks until out_f16 is filled and releases the ticket.  The upload of ticket n+1
 * overlaps the kernels of ticket n, so a caller that submits batch n+1 before it waits for batch n (the Runner in
 * clip-retrieval_amd/runner.py) keeps the GPU busy across batches.  `pixels` / `ids` must stay valid until clipx_wait()
 * when they are page-locked (they are uploaded in place); pageable memory is copied during the call.  At most 4 tickets
 * can be outstanding per handle (CLIPX_E_STATE otherwise).  Every ticket must be waited for exactly once. */
typedef struct clipx_ticket clipx_ticket;
int clipx_encode_image_async(clipx_handle* h, const void* pixels, int B, int pix_fmt, uint16_t* out_f16, clipx_ticket** ticket);
int clipx_encode_text_async(clipx_handle* h, const int32_t* ids, int B, uint16_t* out_f16, clipx_ticket** ticket);
int clipx_wait(clipx_ticket* ticket);

/* Same with every buffer already resident in HBM (benchmark path, and callers that do their own
 * hipMemcpyAsync double-buffering).  `stream` is a hipStream_t (NULL = the handle's stream);
 * asynchronous on that stream.  out_f32_or_null: optional f32 [B, embed_dim] copy of the
 * normalised embedding before the fp16 rounding (parity tests measure cosine on it).  The handle's activation workspace
 * is shared by all calls: consecutive calls are ordered by an event even when they use different streams.
 * clipx_encode_text_device with B > 8 synchronises `stream` ONCE before its kernels are queued: it reads the token ids back
 * to find every caption's EOT position, and then runs the (causal) text tower on the rows up to the EOT only -- the same
 * embeddings, bit for bit (CLIPX_OPT_RAGGED_TEXT = 0 / environment CLIPX_RAGGED_TEXT=0: every row, and a fully asynchronous
 * call; a call on a `stream` that is being captured into a hipGraph takes that path by itself, with or without host ids).  Capturing
 * these calls into a caller's own hipGraph is allowed for B > 8 (smaller batches replay the library's own graphs); the replays
 * share the handle's activation workspace, so they must not run concurrently with other calls on the handle. */
int clipx_encode_image_device(clipx_handle* h, const void* pixels_dev, int B, int pix_fmt, uint16_t* out_f16_dev,
                              float* out_f32_or_null, void* stream);
int clipx_encode_text_device(clipx_handle* h, const int32_t* ids_dev, int B, uint16_t* out_f16_dev,
                             float* out_f32_or_null, void* stream);
/* The same for a caller that ALSO holds the ids on the host -- the reference's batch does: item["text_tokens"] is a CPU tensor the
 * reader tokenised (reader.py:163-170, mapper.py:63-65), uploaded by the caller for its own double-buffering.  ids_host [B, ctx_len]
 * must equal ids_dev and stay valid for the duration of the call; the EOT positions are taken from it, so nothing is read back and
 * the call never synchronises `stream`. */
int clipx_encode_text_device_ids(clipx_handle* h, const int32_t* ids_dev, const int32_t* ids_host, int B, uint16_t* out_f16_dev,
                                 float* out_f32_or_null, void* stream);

/* The geometric half of the reference's image transform on the GPU (reader.py:83,87 `self.image_transform(image)` = CLIP's
 * Resize(S, BICUBIC) + CenterCrop(S) on a PIL image), bit-identical to Pillow's 8-bit bicubic resample: B decoded RGB images of
 * any sizes, packed in one device buffer (image i = uint8 [hw[2i], hw[2i+1], 3] at byte offset offsets[i]), become the uint8
 * [B, S, S, 3] batch that clipx_encode_image_device takes as CLIPX_PIX_U8_NHWC.  offsets / hw are HOST arrays; the filter weights
 * are computed on the host in Pillow's arithmetic (a few KB per image), the pixel work runs on `stream` (asynchronous).
 * CLIPX_E_UNSUPPORTED for down-scales beyond ~30 x (a band of output rows no longer fits the LDS). */
int clipx_resize_crop_u8_device(int device, const void* src_dev, const int64_t* offsets, const int32_t* hw, int B, int S, void* out_dev,
                                void* stream);

/* Baseline JPEG decode in two stages, for ONE class of files -- SOF0, 8-bit, one interleaved scan (DRI / RSTn allowed),
 * grayscale or JFIF YCbCr 4:4:4 / 4:2:2 / 4:2:0, both sides <= max_side -- and bit-identical to Pillow's (libjpeg's default)
 * decode of them.  Every other file, and every file that does not parse cleanly to its EOI, is DEFERRED: not an error, the
 * caller decodes it as it did before.
 *
 * Entropy stage, HOST only (no HIP call: usable in a process without a GPU).  clipx_jpeg_probe_host parses up to the SOF and
 * returns the class, the descriptor and the size of the record; clipx_jpeg_entropy_host decodes the file into `record`
 * (record_bytes >= the probed size; never written past it):
 *   uint16 qt[3][64]         each component's quantisation table
 *   int16  coef[blocks][64]  component 0's blocks, then 1's, then 2's; a component's blocks in raster order of its plane padded
 *                            to whole MCUs (bw[c] x bh[c]), DC prediction undone
 * both in NATURAL order (index = 8 * row + column).  Return: CLIPX_JPEG_TAKEN, CLIPX_JPEG_DEFERRED (nothing was written: neither
 * the descriptor nor the record), or CLIPX_E_ARG. */
#define CLIPX_JPEG_DEFERRED 0
#define CLIPX_JPEG_TAKEN 1
typedef struct {
  int32_t width, height;
  int32_t ncomp;        /* 1 = grayscale, 3 = YCbCr */
  int32_t hs, vs;       /* luma sampling factors, 1 or 2 (chroma is 1 x 1) */
  int32_t bw[3], bh[3]; /* blocks per row / column of each component's padded plane */
  int32_t blocks;       /* of all components */
  int32_t restart;      /* MCUs per restart interval (informative) */
  int32_t pad;
  int64_t coef_off;     /* byte offset of the image's record in the buffer handed to clipx_jpeg_pixels_device: set by the
                           caller that packs the records, a multiple of 16 */
} clipx_jpeg_desc;
int clipx_jpeg_probe_host(const void* data, size_t n, int max_side, clipx_jpeg_desc* desc, size_t* record_bytes);
int clipx_jpeg_entropy_host(const void* data, size_t n, int max_side, clipx_jpeg_desc* desc, void* record, size_t record_bytes);

/* Pixel stage: dequantisation, libjpeg's slow-integer inverse DCT, fancy chroma upsampling and JFIF colour conversion on the GPU
 * (csrc/jpeg_kernels.hip).  coefs_dev holds the B records at descs[i].coef_off (16-byte aligned buffer); image i is written as packed
 * RGB uint8 [height, width, 3] at byte offset offsets[i] of pixels_dev -- the layout clipx_resize_crop_u8_device reads -- and not a byte
 * outside it.  descs / offsets are HOST arrays; asynchronous on `stream`. */
int clipx_jpeg_pixels_device(int device, const void* coefs_dev, const clipx_jpeg_desc* descs, int B, void* pixels_dev,
                             const int64_t* offsets, void* stream);

/* Huffman stage on the device (`gpu_huffman`; csrc/jpegx_scan.h, csrc/jpeg_huff_kernels.hip), same class of files, same verdicts.
 *
 * Host preparation (no HIP call).  clipx_jpeg_scan_probe_host parses up to the SOS and returns the descriptor and the size of the
 * file's SCAN RECORD; clipx_jpeg_scan_host walks the entropy-coded bytes for markers only (no Huffman decoding) and writes the
 * record into `scan` (scan_bytes >= the probed size; never written past it): a header, the quantisation tables, the Huffman tables
 * the scan selects, the table of restart intervals and the file's bytes.  Return as above: TAKEN, DEFERRED (nothing was written --
 * also where the probe took the file and the marker walk does not), or CLIPX_E_ARG.
 *
 * clipx_jpeg_entropy_device decodes B scan records, one wave per restart interval.  scans_dev holds record i in
 * [scan_offs[i], scan_offs[i + 1]) -- scan_offs is a HOST array of B + 1 multiples of 16 -- and image i's output, exactly the record
 * clipx_jpeg_pixels_device reads (uint16 qt[3][64] | int16 coef[blocks][64]), is written at descs[i].coef_off of coefs_dev (HOST
 * descriptors, as the preparation wrote them, coef_off set by the caller).  status_dev[i] (device int32 [B]) becomes 0 when every
 * interval of image i decoded cleanly -- its record then equals clipx_jpeg_entropy_host's byte for byte -- and a reason code > 0
 * otherwise: clipx_jpeg_entropy_host defers exactly those files, their records hold no meaning, and the caller decodes them as it
 * did before.  Nothing outside the B records and the status array is written.  Asynchronous on `stream`; B = 0 is a no-op. */
int clipx_jpeg_scan_probe_host(const void* data, size_t n, int max_side, clipx_jpeg_desc* desc, size_t* scan_bytes);
int clipx_jpeg_scan_host(const void* data, size_t n, int max_side, clipx_jpeg_desc* desc, void* scan, size_t scan_bytes);
int clipx_jpeg_entropy_device(int device, const void* scans_dev, const clipx_jpeg_desc* descs, const int64_t* scan_offs, int B,
                              void* coefs_dev, int32_t* status_dev, void* stream);

/* Split decode inside a restart interval (`huffman_split`; csrc/jpegx_split.h, csrc/jpeg_split_kernels.hip).  A file
 * without restart markers is ONE interval, which clipx_jpeg_entropy_device gives one wave.  With split_bytes != 0 an interval of at
 * least 2 x split_bytes entropy-coded bytes is cut into sub-sequences of split_bytes (doubled until there are at most 512), which
 * one workgroup decodes concurrently: each starts from a guessed state and is decoded again from its predecessor's exit state until
 * a round changes nothing (self-synchronisation), then one more pass writes the coefficients.  Records, statuses and verdicts are
 * those of clipx_jpeg_entropy_device, byte for byte and code for code.  An interval that has not reached the fixed point after
 * max_rounds rounds (periodic content never does before its last sub-sequence) is decoded serially, with the same result.
 *   split_bytes  0 (no interval is split: exactly clipx_jpeg_entropy_device) or a power of two 32 .. 1024
 *   max_rounds   0 = the library's default (16), else >= 1
 *   reserved     must be 0
 * rounds_dev (device int32 [B], or NULL) / *rounds: 0 -- no interval of the image was split; r >= 2 -- the most rounds a split
 * interval of the image took, the round in which nothing decodes counted; -r -- at least one interval gave up after r = max_rounds
 * rounds and was decoded serially.  Nothing outside the B records, the status array and rounds_dev is written.
 * clipx_jpeg_entropy_split_host runs the same decoder on the host with the lanes as a loop, on ONE scan record (16-byte aligned, as
 * clipx_jpeg_scan_host wrote it, with its descriptor): no HIP call, usable without a GPU.  `record` (record_bytes >= the
 * descriptor's record) receives [tables | coefficients], *status and *rounds what the device entry writes for that image. */
typedef struct { int32_t split_bytes; int32_t max_rounds; int32_t reserved[2]; } clipx_jpeg_split;
int clipx_jpeg_entropy_split_device(int device, const void* scans_dev, const clipx_jpeg_desc* descs, const int64_t* scan_offs,
                                    int B, void* coefs_dev, int32_t* status_dev, const clipx_jpeg_split* split,
                                    int32_t* rounds_dev /* [B] or NULL */, void* stream);
int clipx_jpeg_entropy_split_host(const void* scan, size_t scan_bytes, const clipx_jpeg_desc* desc, const clipx_jpeg_split* split,
                                  void* record, size_t record_bytes, int32_t* status, int32_t* rounds);

/* Range guard.  The encoder keeps the residual stream of both towers in IEEE fp16: exact for every checkpoint that is
 * trained or served in fp16 (the reference's CUDA path runs the whole model in fp16, mapper.py:35-41), but a model whose
 * activations exceed 65 504 (possible for bf16-trained checkpoints) would overflow to inf, and LayerNorm turns a row holding inf
 * into a finite-looking WRONG embedding.  Every state of the stream is therefore checked on the device (one compare inside the
 * kernels that read it anyway) and an overflow is reported, never hidden: the host entry points (clipx_encode_image / _text /
 * _f32) and clipx_wait() return CLIPX_E_RANGE for a call in which any row overflowed (the output buffer of that call must be
 * discarded); after *_device calls, clipx_range_check(h, stream) synchronises `stream` and returns CLIPX_OK or CLIPX_E_RANGE for
 * everything queued through the *_device entry points since the previous check (it also clears the flag). */
int clipx_range_check(clipx_handle* h, void* stream);

/* Per-handle switches (defaults in brackets; the environment variables CLIPX_RAGGED_TEXT / CLIPX_FULL_LAST_BLOCK set the initial
 * values).  Both change which rows are computed, never the bytes of the embeddings (tests/test_clip_gpu.py).
 *   CLIPX_OPT_RAGGED_TEXT [1]      text batches > 8 run every layer on the rows up to each caption's EOT only
 *   CLIPX_OPT_POOL_LAST_BLOCK [1]  the last block runs past its attention on the pooled rows only
 *   CLIPX_OPT_PROF_MARKERS [0]     clipx_profile_enable brackets the GEMMs with marker events around each launch, as it does the
 *                                  other kinds, instead of the clock stamps the GEMM kernels write themselves (A/B of the two)
 * clipx_get_option returns the value or -1. */
#define CLIPX_OPT_RAGGED_TEXT 1
#define CLIPX_OPT_POOL_LAST_BLOCK 2
#define CLIPX_OPT_PROF_MARKERS 3
int clipx_set_option(clipx_handle* h, int option, int value);
int clipx_get_option(const clipx_handle* h, int option);

/* Largest batch one launch sequence handles (workspace is sized for it at create time;
 * CLIPX_MAX_BATCH env var, default 256).  Bigger B is processed in chunks of this size. */
int clipx_max_batch(const clipx_handle* h);
/* Number of small-batch launch sequences this handle has captured as hipGraphs so far (batches of <= 8 samples -- the B = 1
 * query encode of KnnService.compute_query, clip_back.py:207-255 -- are replayed from a graph per (tower, B, buffers, stream));
 * introspection for tests and service dashboards. */
int clipx_graphs_cached(const clipx_handle* h);
/* Rows the text tower ran its layers on in the latest text chunk of this handle: B * ctx_len for a rectangular batch, the
 * sum of the caption lengths for a ragged one -- rounded up to a multiple of 256 where the batch is large enough for the
 * 256-row GEMM tiles (the extra rows repeat real rows and are never read); introspection for tests. */
int clipx_last_text_rows(const clipx_handle* h);
int clipx_embed_dim(const clipx_handle* h);

/* Raw bf16 GEMM of this library (out[m,n] = sum_k A[m,k] W[n,k] + bias[n]), device pointers;
 * exposed so tests and bench.py can check / time the dominant kernel in isolation.
 * epi: 0 bias->bf16, 1 bias+quick_gelu->bf16, 2 bias+gelu->bf16, 3 f32 out += acc+bias. */
int clipx_gemm_bf16_device(int device, const void* A_bf16, const void* W_bf16, const float* bias, void* out, int M,
                           int N, int K, int epi, void* stream);

/* The same with the two extras the encoder's LayerNorm-folded layers use: rowscale_or_null f32 [M] (epi 0..2:
 * out = act(acc * rowscale[m] + bias[n]); null = ones) and out16_or_null bf16 [M, N] (epi 3: also the bf16 rounding of the
 * new f32 rows -- the shadow of the residual stream the next folded GEMM reads). */
int clipx_gemm_bf16_ex_device(int device, const void* A_bf16, const void* W_bf16, const float* bias, void* out, int M, int N,
                              int K, int epi, const float* rowscale_or_null, void* out16_or_null, void* stream);
/* (the _ex entry point also takes epi 6: out is IEEE fp16 [M, N], updated in place, out = fp16(f32(out) + acc + bias) -- the
 * residual epilogue of out_proj / fc2 in the encoder, whose residual stream is stored in fp16.) */

/* The LayerNorm-folded GEMMs of the encoder (QKV, fc1) read that fp16 residual stream as their A operand: A and W are IEEE
 * fp16 (v_mfma_f32_32x32x16_f16, the same rate as bf16), out bf16 [M, N]; epi 0..2 and rowscale as above, or epi 7: epi 0 with
 * an IEEE fp16 output (the QKV projection: q and k carry three more mantissa bits into the softmax logits). */
int clipx_gemm_f16_device(int device, const void* A_f16, const void* W_f16, const float* bias, void* out_16bit, int M, int N, int K,
                          int epi, const float* rowscale_or_null, void* stream);

/* The same GEMM as the encoder's folded layers run it since round 6 (mapper.py:57,65 -> the LayerNorm in front of QKV / fc1): the row
 * scales are NOT an input but 1 / sqrt(var(A[m, :]) + eps) of the fp16 rows of A itself (K = the row length), computed inside the
 * 4-wave 256x256 kernel for the rows it multiplies and by the statistics pass into rstd_buf [M] (scratch; only those rows are
 * written) for the others -- the same bits either way (csrc/gemm_common.h: ln_rstd_onepass). */
int clipx_gemm_f16_ln_device(int device, const void* A_f16, const void* W_f16, const float* bias, void* out_16bit, int M, int N, int K,
                             int epi, float* rstd_buf, float eps, void* stream);

/* The attention and LayerNorm kernels in isolation (device pointers), for per-kernel parity tests:
 * qkv IEEE fp16 [B*T, 3*H*64] (q | k | v as the QKV projection's epi 7 writes them; the products run on fp16 MFMA, P is
 * rounded to fp16) -> out bf16 [B*T, H*64];  x f32 [M, d] -> y (bf16 if out_bf16 else f32). */
int clipx_attention_device(int device, const void* qkv_f16, void* out_bf16, int B, int T, int H, int causal,
                           void* stream);
/* Same for head dimension dh = 64, 80 (ViT-H/14 image tower: 1280 / 16), 88 (ViT-g/14: 1408 / 16) or 104 (ViT-bigG/14: 1664 / 16):
 * qkv [B*T, 3*H*dh] -> out [B*T, H*dh].  dh = 88 and 104: not causal, T <= 96 or 257 .. 288 (CLIPX_E_UNSUPPORTED otherwise). */
int clipx_attention_dh_device(int device, const void* qkv_f16, void* out_bf16, int B, int T, int H, int dh,
                              int causal, void* stream);
/* The same kernels with the two arguments the encoder itself passes them, for per-kernel tests of those forms.
 *   q_blocks  0: every row.  n > 0: only the rows of the n leading blocks of 32 queries of every sample are computed (the pooled
 *             last block asks for 1); those rows hold the bits of the full launch, the OTHER ROWS OF out ARE UNSPECIFIED.
 *   offs_dev_or_null, lens_dev_or_null  device int32 [B], both or neither (CLIPX_E_ARG otherwise): a ragged batch, sample b owns
 *             the lens[b] >= 1 packed rows from row offs[b] on, so qkv and out hold sum(lens) rows and T is the longest length.
 *             Head dimension 64 and T <= 128 only (CLIPX_E_UNSUPPORTED otherwise).
 * The limits of T are those of the two entry points above; dh = 80, 88 and 104 have no kernel at T = 97 .. 256, dh = 88 and 104 none
 * that is causal or ragged (CLIPX_E_UNSUPPORTED);
 * a refused call launches nothing. */
int clipx_attention_ex_device(int device, const void* qkv_f16, void* out_bf16, int B, int T, int H, int dh, int causal,
                              int q_blocks, const int32_t* offs_dev_or_null, const int32_t* lens_dev_or_null, void* stream);
/* d: a multiple of 128, at most 2048 (here and in clipx_rowstats_device); out_bf16 = 2: IEEE fp16 rows */
int clipx_layernorm_device(int device, const float* x, const float* gamma, const float* beta, void* y, int out_bf16,
                           int M, int d, float eps, void* stream);
/* LayerNorm statistics of the residual stream as the LayerNorm-folded GEMMs consume them (per-kernel parity test):
 * rstd[m] = 1 / sqrt(var(x16[m, :]) + eps) by a pass over the 16-bit rows (is_f16: IEEE fp16, else bf16; is_f16 = 2: fp16 rows by the
 * one-pass canonical form that clipx_gemm_f16_ln_device uses for the rows its 4-wave kernel does not take). */
int clipx_rowstats_device(int device, const void* x16, int is_f16, float* rstd, int M, int d, float eps, void* stream);

/* The embedding tail in isolation (per-kernel parity test): pooled rows x IEEE fp16 [B, d] -> LayerNorm(gamma, beta) -> @ proj^T
 * (bf16 [E, d]) -> / L2 norm -> out_f16 [B, E] (+ the f32 rows); scratch: B * E floats.  rows_per_workgroup selects the projection
 * kernel: 0 the per-sample one (small batches, queries), 8 or 16 the batched one -- every choice writes the same bytes;
 * CLIPX_E_UNSUPPORTED where the batched kernel cannot hold that many rows of d floats.  rows_per_workgroup < 0 launches nothing
 * and RETURNS the value the encoder itself uses for a batch of this (B, d, E): 0 or 8. */
int clipx_tail_device(int device, const void* x_f16, const float* gamma, const float* beta, const void* proj_bf16, uint16_t* out_f16,
                      float* out_f32_or_null, float* scratch, int B, int d, int E, float eps, int rows_per_workgroup, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Multilingual text towers (the reference's `use_mclip`: clip_inference/mapper.py:44-47, 62-63 and clip_back.py:222-224, 837-859).
 * One family: a post-LN, bidirectional, padding-masked BERT encoder -> masked mean pooling -> one dense layer -> unit L2 norm.
 *   x = LN_emb(word[id] + pos[pos_offset + t]);  per layer: x = LN_att(x + out_proj(attention(qkv(x)))), x = LN_out(x + fc2(gelu(fc1(x))))
 *   y = dense(mean over the sample's tokens of x) (+ bias);  out = y / |y|
 * DistilBERT multilingual (sentence-transformers/clip-ViT-B-32-multilingual-v1): 6 layers, width 768, 12 heads, mlp 3072, vocab
 * 119 547, 512 positions, eps 1e-12, dense 768 -> 512 without bias.  XLM-R large (M-CLIP XLM-Roberta-Large-Vit-L-14 / -Vit-B-32): 24
 * layers, width 1024, 16 heads, mlp 4096, vocab 250 002, 514 positions from 2 on, eps 1e-5, dense 1024 -> 768 or 512 with bias.
 * (Shapes recalled from memory of the published configurations; a loader takes the true values from the checkpoint's config.json.)
 * Arithmetic: the residual stream is IEEE fp16 and every LayerNorm rewrites it in place from fp32 statistics; QKV and fc1 read it as
 * fp16 MFMA operands, out_proj and fc2 run on bf16 operands and add into it in fp32 (epilogue 6); the pooled mean, the dense layer
 * (f32 weights) and the norm are fp32.  erf-GELU.  Head dimension 64 and at most 128 tokens per text (the ragged attention kernels). */
typedef struct clipx_bert clipx_bert;
typedef struct clipx_bert_desc {
  int vocab;      /* 119547 | 250002 */
  int max_pos;    /* rows of the position table: 512 | 514 */
  int pos_offset; /* position row of token 0: 0 | 2 (XLM-R: padding_idx + 1) */
  int width;      /* 768 | 1024: a multiple of 128, at most 2048 */
  int layers;     /* 6 | 24 */
  int heads;      /* 12 | 16: width / heads must be 64 */
  int mlp;        /* 3072 | 4096: a multiple of 128 */
  int out_dim;    /* 512 | 768: rows of the dense layer */
  int dense_bias; /* 0 | 1 */
  int max_len;    /* tokens per text, at most 128; pos_offset + max_len <= max_pos */
  float ln_eps;   /* 1e-12 | 1e-5 */
} clipx_bert_desc;

/* Number of floats in the weight blob for `desc`.  Blob order, all row-major, torch `nn.Linear` [out, in] weights:
 *   word embeddings [vocab, width]; position table [max_pos, width] (XLM-R: its single token-type row already added to every row);
 *   embedding LN {w, b}; per layer { in_proj [3 width, width] (q | k | v), its bias [3 width]; out_proj {w [width, width], b};
 *   attention LN {w, b}; fc1 {w [mlp, width], b}; fc2 {w [width, mlp], b}; output LN {w, b} }; dense weight [out_dim, width];
 *   dense bias [out_dim] when dense_bias. */
size_t clipx_bert_blob_floats(const clipx_bert_desc* desc);
/* CLIPX_E_UNSUPPORTED: head dimension other than 64, max_len > 128, a width that is not a multiple of 128 or above 2048, an mlp width
 * that is not a multiple of 128.  The blob is consumed during the call. */
int clipx_bert_create(const clipx_bert_desc* desc, const float* blob, size_t blob_floats, int device, clipx_bert** out);
void clipx_bert_destroy(clipx_bert* h);
int clipx_bert_out_dim(const clipx_bert* h);

/* ids: host int32 [B, max_len], left-aligned; only the first lens[b] ids of row b are read (the attention mask of the reference's
 * tokenizers is 1 on a prefix).  lens: host int32 [B], each in 1 .. max_len (CLIPX_E_ARG otherwise: nothing is launched).
 * out_f32: host [B, out_dim] unit-norm rows; out_f16_or_null: their IEEE fp16 rounding.  Any B >= 1 (chunked internally).
 * CLIPX_E_RANGE when the fp16 residual stream overflowed (the outputs of the call must be discarded).  Calls on one handle serialise. */
int clipx_bert_encode(clipx_bert* h, const int32_t* ids, const int32_t* lens, int B, float* out_f32, uint16_t* out_f16_or_null);
/* The same with ids and outputs resident in HBM, asynchronous on `stream` (NULL = the handle's stream); lens_host as above, read
 * during the call.  clipx_bert_range_check synchronises `stream` and reports / clears the range flag of the calls since the last check. */
int clipx_bert_encode_device(clipx_bert* h, const int32_t* ids_dev, const int32_t* lens_host, int B, float* out_f32_dev,
                             uint16_t* out_f16_dev_or_null, void* stream);
int clipx_bert_range_check(clipx_bert* h, void* stream);

/* The three kernels of the family in isolation (device pointers), for per-kernel parity tests.
 * embed: ids int32, offs / lens int32 [B] (sample b owns the packed rows offs[b] .. offs[b] + lens[b] - 1 of out, IEEE fp16
 *   [rows, d]); ids_stride > 0: ids is [B, ids_stride] and only the first lens[b] of a row are read; 0: ids is packed like the rows.
 *   T = the longest length; row offs[b] + t = LN(word[id] + pos[pos_offset + t]) gamma + beta; an id outside [0, vocab) is clamped.
 *   CLIPX_E_ARG unless 1 <= T, pos_offset + T <= max_pos.  d: a multiple of 128, at most 2048 (here and in postln).
 * postln: x16 IEEE fp16 [M, d] in place, fp32 two-pass statistics; a row of equal elements gives exactly fp16(beta).
 * pool: x16 IEEE fp16 packed rows; y_raw f32 [B, E] receives W mean(rows) (+ bias) (W f32 [E, d], fp32 accumulation), out_f32 [B, E]
 *   = y / |y| (|y| = 0 -> 1), out_f16_or_null its fp16 rounding.  d: a multiple of 32, at most 2048. */
int clipx_bert_embed_device(int device, const int32_t* ids, int ids_stride, const int32_t* offs, const int32_t* lens, int B, int T,
                            int rows, const float* word, const float* pos, int pos_offset, int max_pos, const float* gamma,
                            const float* beta, void* out_f16, int d, int vocab, float eps, void* stream);
int clipx_postln_f16_device(int device, void* x16, const float* gamma, const float* beta, int M, int d, float eps, void* stream);
int clipx_bert_pool_device(int device, const void* x16, const int32_t* offs, const int32_t* lens, const float* W,
                           const float* bias_or_null, float* y_raw, float* out_f32, uint16_t* out_f16_or_null, int B, int d, int E,
                           void* stream);

/* Live per-kernel timing for bench.py: launches of the enabled kinds are bracketed by hipEvents on
 * their stream.  kind: 0 gemm, 1 attention, 2 layernorm, 3 other.  on: 0 off, 1 all kinds, else a bit
 * mask with bit (kind + 1): 2 = GEMMs only, 4 | 8 | 16 = everything but the GEMMs.  get() sums and resets. */
int clipx_profile_enable(clipx_handle* h, int on);
int clipx_profile_get(clipx_handle* h, int kind, int64_t* launches, double* ms, double* flops);
/* The GEMMs (kind 0) are timed by the kernels themselves: every kernel of a GEMM launch stamps its first start and its last end
 * (constant-rate device counter) into a slot of device memory the handle owns, and a GEMM launch counts once, with the sum over
 * its kernels of last end - first start (CLIPX_OPT_PROF_MARKERS = 1: events recorded around the launch, like the other kinds).
 * The slots are allocated in chunks, the first one by clipx_profile_enable; clipx_profile_get synchronises the streams the GEMMs
 * ran on, reads the slots once and hands them back; CLIPX_E_STATE when a profiled GEMM launched no kernel or left a slot unwritten.
 * The events of the marker form come from a pool on the handle that clipx_profile_get refills; clipx_profile_events = events
 * created so far (the stamp form creates none). */
int clipx_profile_events(const clipx_handle* h);
/* Test entry: one GEMM on the caller's device buffers through the handle's profiler, the way the encoder issues its own (one scope
 * of 2 M N K flops; epi / f16 / rowscale as in clipx_gemm_*_device, table [T, N] for epilogue 4).  CLIPX_E_ARG for a null operand,
 * a null table or T <= 0 with epilogue 4, a null bias with any other.  What the GEMM launcher refuses returns CLIPX_E_HIP and
 * leaves a scope without kernels behind. */
int clipx_profile_gemm_device(clipx_handle* h, const void* A, const void* W, const float* bias_or_null, void* out,
                              const float* table_or_null, int T, int M, int N, int K, int epi, int f16,
                              const float* rowscale_or_null, void* stream);

const char* clipx_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* CLIPX_H */
