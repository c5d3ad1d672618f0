// clipx_encode.hip -- the launch sequence of one chunk of either CLIP tower (clipx_host.h: vision_chunk / text_chunk): the layer
// driver, the ragged text batch, the hipGraph replay of small batches, and the event brackets of clipx_profile_*.

#include "clipx_host.h"

using namespace clipx;

// ---------------------------------------------------------------------------------------------
// launch helpers with optional event bracketing
// ---------------------------------------------------------------------------------------------
// Timing events live in a pool on the handle: a scope takes what it needs, clipx_profile_get returns what it has read.
static hipEvent_t prof_take(Profiler& p) {
  if (!p.unused.empty()) {
    hipEvent_t e = p.unused.back();
    p.unused.pop_back();
    return e;
  }
  Event e;
  if (e.create() != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  p.created.push_back(std::move(e));
  return p.created.back();
}

// Brackets the launches of one scope when its kind is being profiled.  GEMMs (kind 0) get the stamp form: events() is handed to
// launch_gemm through GemmArgs, every kernel it launches takes the next free slot of the profiler as an argument and writes its own
// first start and last end into it (gemm_common.h stamp_start / stamp_end) -- the dispatches are plain launches that carry nothing,
// and nothing is recorded on the stream.  (Two marker packets around each of the ~136 GEMM launches of a step kept back-to-back
// dispatches apart and cost 1.1 ms of a 43.7 ms ViT-L/14 step; a completion signal with timestamps on each dispatch 0.5 ms of 42.0:
// DESIGN 5.)  The other kinds, CLIPX_OPT_PROF_MARKERS, and a stream that is being captured keep the marker form.
struct ProfScope {
  Profiler& p;
  hipStream_t st;
  ProfEvent e{};
  LaunchEvents le{};
  bool on = false;
  ProfScope(clipx_handle* h, hipStream_t st_, int kind, double flops) : p(h->prof), st(st_) {
    if (!(p.mask & (1 << kind))) return;
    e.kind = kind;
    e.flops = flops;
    e.st = st;
    e.stamps = kind == 0 && !p.markers && !stream_is_capturing(st);
    if (e.stamps) {
      e.slot0 = p.book.in_use();
      le = LaunchEvents{this, &ProfScope::next_slot};
      on = true;
      return;
    }
    for (int i = 0; i < 2; ++i) {
      e.ev[i] = prof_take(p);
      if (!e.ev[i]) {  // no event to be had: this scope goes untimed
        while (i > 0) p.unused.push_back(e.ev[--i]);
        return;
      }
    }
    on = true;
    (void)hipEventRecord(e.ev[0], st);
  }
  // The next kernel's slot.  Only when the chunks have run out is anything allocated here: one more chunk, filled and synchronised
  // (add_chunk) before any of its slots is handed out.
  static StampSlot* next_slot(void* self) {
    ProfScope& s = *static_cast<ProfScope*>(self);
    int id = s.p.book.take();
    if (id < 0) {
      if (s.p.add_chunk(s.st) != hipSuccess) {
        (void)hipGetLastError();
        s.p.starved = true;
        return nullptr;
      }
      id = s.p.book.take();
    }
    ++s.e.nslots;
    return s.p.slot(id);
  }
  LaunchEvents* events() { return on && e.stamps ? &le : nullptr; }
  ~ProfScope() {
    if (!on) return;
    if (!e.stamps) (void)hipEventRecord(e.ev[1], st);
    p.scopes.push_back(e);
  }
};

// launch_gemm as one profiled scope of `flops` (run_gemm below; the test entry clipx_profile_gemm_device, clipx_hooks.hip)
int clipx::profiled_gemm(clipx_handle* h, GemmArgs& g, hipStream_t st, double flops) {
  ProfScope ps(h, st, 0, flops);
  g.events = ps.events();
  HIPCHK(launch_gemm(g, st));
  return 0;
}

static int run_gemm(clipx_handle* h, const Call& c, const bf16* A, const bf16* W, const float* bias, void* out,
                    const float* table, int T, int M, int N, int K, int epi, const float* rowscale = nullptr, bool f16 = false,
                    float stats_eps = 0.f, int pad_rows = 0) {
  GemmArgs g{};
  g.A = A; g.W = W; g.bias = bias; g.out = out; g.table = table; g.T = T;
  g.M = M; g.N = N; g.K = K; g.epi = epi; g.variant = h->gemm_variant; g.n_cu = h->n_cu; g.row0 = 0;
  g.rowscale = rowscale; g.out16 = nullptr; g.f16 = f16 ? 1 : 0;
  // stats_eps > 0: a LayerNorm-folded GEMM that computes the row scales itself -- inside the 4-wave kernel for the rows it takes, by
  // launch_rowstats into `rowscale` for the others (launch_gemm decides)
  g.stats_eps = stats_eps; g.range_flag = stats_eps > 0.f ? c.range_flag : nullptr;
  // split-K only on the single-query path (B == 1, KnnService.compute_query): every batch of two or more samples is computed
  // by the unsplit kernels, whose rows do not depend on the batch they travel in (bitwise); a B = 1 row differs from the same
  // sample inside a batch by f32 summation order only
  if (c.single_query) { g.splitk_ws = h->ws.splitk; g.splitk_ws_bytes = h->ws.splitk_bytes; }
  return profiled_gemm(h, g, c.st, 2.0 * (M - pad_rows) * (double)N * K);  // (pad rows of a ragged text batch are not work the model asks for)
}

// where run_layers leaves the pooled rows (fp16 [B, width]) when it pools the last block: behind the gathered attention rows
static void* pooled_rows(const clipx_handle* h, int B, int width) {
  return reinterpret_cast<char*>(h->ws.x.p) + (((size_t)B * width * sizeof(bf16) + 255) & ~(size_t)255);
}

struct Ragged {  // device arrays of one ragged text batch (see clipx_handle::ragged_text)
  int M;                // rows in all: sum of the lengths, pad rows included (clipx_ragged_plan.h)
  int rows;             // the real rows among them (what the profile's flop counts are taken from)
  int S;                // samples the attention sees: B + the pseudo-samples that own the pad rows
  const int* offs;      // [S] first row of sample b
  const int* lens;      // [S] rows of sample b (EOT position + 1)
  const int* rowmap;    // [M] compact row -> b * ctx_len + t
  const int* poolrows;  // [B] compact row of the EOT token
  double att_flops;     // 4 heads dh sum(len^2)
};

// Returns in *pooled whether the residual stream that leaves the last block is the compact [B, width] buffer of pooled rows
// (ws.x reused) instead of ws.xn [B * T, width].
static int run_layers(clipx_handle* h, const Call& c, const Tower& t, int B, int causal, const int32_t* ids, bool* pooled,
                      const Ragged* rg = nullptr) {
  const Workspace& ws = h->ws;
  hipStream_t st = c.st;
  const int M = rg ? rg->M : B * t.T, w = t.width;
  const int pad = rg ? rg->M - rg->rows : 0;
  const float eps = h->desc.ln_eps;
  const int act = h->desc.act == CLIPX_ACT_QUICK_GELU ? EPI_BIAS_QGELU_BF16 : EPI_BIAS_GELU_BF16;
  // On entry ws.xn holds the residual stream x in fp16 (written by ln_pre / the text embedding).  Per block:
  //   rstd = rowstats(x);    qkv = fp16((x @ Wqkv'^T) * rstd + c_qkv)      [= LN1(x) @ Wqkv^T + b: LayerNorm folded; fp16 MFMA, fp16 out]
  //   att = attention(qkv);  x = fp16(x + att @ Wout^T + b_out)            [in place, bf16 MFMA, f32 add]
  //   rstd = rowstats(x);    h = act((x @ Wfc1'^T) * rstd + c_fc1);  x = fp16(x + h @ Wfc2^T + b_fc2)
  // (LayerNorm partial statistics computed by the residual epilogues instead of the rowstats pass were built twice in round 3
  // and measured slower on the same box -- the extra epilogue work costs more GEMM time than the 134 MB re-read it saves:
  // the patch is in the repository's history, round 3)
  for (int l = 0; l < t.layers; ++l) {
    const LayerW& L = t.L[l];
    int r;
    // (LayerNorm statistics: the separate pass of rounds 2 - 5, or with CLIPX_LN_FUSED=1 inside the GEMM -- run_gemm's stats_eps)
    if (!h->ln_fused) { ProfScope ps(h, st, 2, 0); HIPCHK(launch_rowstats(ws.xn, ws.rstd, M, w, eps, st, 1, c.range_flag)); }
    if ((r = run_gemm(h, c, ws.xn, L.qkv_w, L.qkv_c, ws.qkv, nullptr, 1, M, 3 * w, w, EPI_BIAS_F16, ws.rstd, true, h->ln_fused ? eps : 0.f, pad))) return r;
    // last block of the image tower: only token 0's attention row is read afterwards -> query block 0 only (same arithmetic)
    const bool pool_here = l == t.layers - 1 && h->pool_last_block && t.T > 1;
    const int q_blocks = pool_here && !ids ? 1 : 0;
    const double att_rows = q_blocks ? std::min(32, t.T) : t.T;
    { ProfScope ps(h, st, 1, rg ? rg->att_flops * t.heads * (w / t.heads) : 4.0 * B * t.heads * att_rows * t.T * (w / t.heads));
      HIPCHK(launch_attention(ws.qkv, ws.att, rg ? rg->S : B, t.T, t.heads, w / t.heads, causal, st, q_blocks, rg ? rg->offs : nullptr, rg ? rg->lens : nullptr)); }
    if (pool_here) {
      // The embedding reads ONE row of this block's output per sample (token 0 / the EOT token: launch_tail), and past the
      // attention every operation of a block is row-wise: out-proj, both residual adds, LayerNorm 2 and the MLP run on those B
      // rows only.  Same kernels, and a GEMM row does not depend on the rows it travels with (bitwise): the embeddings are the
      // bytes the full block gives (tests/test_clip_gpu.py; CLIPX_FULL_LAST_BLOCK=1 runs the full block).
      bf16* attc = reinterpret_cast<bf16*>(ws.x.p);
      void* xc = pooled_rows(h, B, w);
      { ProfScope ps(h, st, 3, 0); HIPCHK(launch_gather_pooled(ws.att, ws.xn, ids, attc, xc, B, t.T, w, st, rg ? rg->poolrows : nullptr)); }
      if ((r = run_gemm(h, c, attc, L.out_w, L.out_b, xc, nullptr, 1, B, w, w, EPI_BIAS_RESID_H16))) return r;
      if (!h->ln_fused) { ProfScope ps(h, st, 2, 0); HIPCHK(launch_rowstats(xc, ws.rstd, B, w, eps, st, 1, c.range_flag)); }
      if ((r = run_gemm(h, c, reinterpret_cast<const bf16*>(xc), L.fc1_w, L.fc1_c, ws.hbuf, nullptr, 1, B, t.mlp, w, act, ws.rstd, true, h->ln_fused ? eps : 0.f))) return r;
      if ((r = run_gemm(h, c, ws.hbuf, L.fc2_w, L.fc2_b, xc, nullptr, 1, B, w, t.mlp, EPI_BIAS_RESID_H16))) return r;
      *pooled = true;
      return 0;
    }
    if ((r = run_gemm(h, c, ws.att, L.out_w, L.out_b, ws.xn, nullptr, 1, M, w, w, EPI_BIAS_RESID_H16, nullptr, false, 0.f, pad))) return r;
    if (!h->ln_fused) { ProfScope ps(h, st, 2, 0); HIPCHK(launch_rowstats(ws.xn, ws.rstd, M, w, eps, st, 1, c.range_flag)); }
    if ((r = run_gemm(h, c, ws.xn, L.fc1_w, L.fc1_c, ws.hbuf, nullptr, 1, M, t.mlp, w, act, ws.rstd, true, h->ln_fused ? eps : 0.f, pad))) return r;
    if ((r = run_gemm(h, c, ws.hbuf, L.fc2_w, L.fc2_b, ws.xn, nullptr, 1, M, w, t.mlp, EPI_BIAS_RESID_H16, nullptr, false, 0.f, pad))) return r;
  }
  *pooled = false;
  return 0;
}

constexpr int GRAPH_MAX_B = 8;      // batches up to this size are replayed from a captured graph
constexpr size_t GRAPH_MAX = 64;    // graphs kept per handle (distinct buffer sets of callers that bring their own)

// Runs `body` (which only launches kernels on `st`) directly, or -- small batch, profiling off -- through a hipGraph captured
// from exactly that launch sequence the first time this (tower, B, buffers, stream) combination is seen.  Any capture /
// instantiate failure switches graphs off for the handle and runs the plain launches: same kernels, same results.
template <class F>
static int run_graphed(clipx_handle* h, hipStream_t st, const GraphCache::Key& key, int B, F&& body) {
  GraphCache& gc = h->graphs;
  if (!gc.on || h->prof.mask || B > GRAPH_MAX_B) return body();
  auto it = gc.execs.find(key);
  if (it != gc.execs.end()) {
    HIPCHK(hipGraphLaunch(it->second, st));
    return 0;
  }
  if (gc.execs.size() >= GRAPH_MAX) return body();
  if (gc.seen.size() > 4 * GRAPH_MAX) gc.seen.clear();
  if (++gc.seen[key] < 2) return body();
  if (hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) != hipSuccess) {
    (void)hipGetLastError();
    gc.on = false;
    return body();
  }
  const int r = body();
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(st, &g);
  hipGraphExec_t ex = nullptr;
  if (r == 0 && e == hipSuccess && g && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess) {
    (void)hipGraphDestroy(g);
    gc.execs[key] = GraphExec(ex);
    HIPCHK(hipGraphLaunch(ex, st));
    return 0;
  }
  if (g) (void)hipGraphDestroy(g);
  (void)hipGetLastError();
  gc.on = false;
  return body();  // nothing ran during the capture
}

static int vision_chunk_body(clipx_handle* h, const Call& c, const void* pix_dev, int B, int fmt, uint16_t* out_f16, float* out_f32) {
  const clipx_model_desc& d = h->desc;
  const ClipWeights& W = h->w;
  const Workspace& ws = h->ws;
  const Tower& V = W.vis;
  hipStream_t st = c.st;
  const int M = B * V.T;
  { ProfScope ps(h, st, 3, 0); HIPCHK(launch_im2col(pix_dev, fmt, B, d.image_size, d.patch_size, W.Kp, d.pix_mean, d.pix_std, ws.patches, st)); }
  int r = run_gemm(h, c, ws.patches, W.conv_w, nullptr, ws.x, W.clspos, V.T, M, V.width, W.Kp, EPI_TABLE_F32);
  if (r) return r;
  { ProfScope ps(h, st, 2, 0); HIPCHK(launch_layernorm(ws.x, W.ln_pre_w, W.ln_pre_b, ws.xn, 2, M, V.width, d.ln_eps, st)); }
  bool pooled = false;
  if ((r = run_layers(h, c, V, B, 0, nullptr, &pooled))) return r;
  const void* xf = pooled ? pooled_rows(h, B, V.width) : ws.xn.p;
  { ProfScope ps(h, st, 3, 0); HIPCHK(launch_tail(xf, nullptr, V.lnf_w, V.lnf_b, V.proj, out_f16, out_f32, reinterpret_cast<float*>(ws.qkv.p), B, pooled ? 1 : V.T, V.width, d.embed_dim, d.ln_eps, st, 1, c.range_flag)); }
  return 0;
}

// Builds the ragged description of a text batch from its ids (host) in a slot of the ring and uploads it: the lengths by the
// tower's pooling rule, everything else by the planner (clipx_ragged_plan.h: whole m-tiles, pseudo-samples).  Only the attention
// (one more "sample" each) and the row-wise kernels see the pseudo-samples; the pooled rows, gather_pooled and the tail keep B entries.
static int ragged_prepare(clipx_handle* h, hipStream_t st, const int32_t* ids_host, int B, Ragged* rg) {
  const int T = h->w.txt.T, w = h->w.txt.width;
  int s;
  if (int r = h->ragged.take(&s)) return r;
  int* slot = h->ragged.ints(s);
  int M = 0;
  rg->att_flops = 0.0;
  for (int b = 0; b < B; ++b) {
    const int len = slot[b] = ragged_pooled_len(ids_host + (size_t)b * T, T);
    M += len;
    rg->att_flops += 4.0 * (double)len * len;
  }
  const int Mp = gemm256_whole_tile_rows(M, 3 * w, w, h->gemm_variant, h->n_cu);
  const RaggedPlan p = ragged_complete(slot, slot, B, T, Mp, true);
  if (!p.S) return fail(CLIPX_E_ARG, "internal: the ragged slot does not hold the padded text rows");
  if (int r = h->ragged.upload(s, p.ints, st)) return r;
  const int* dev = h->ragged.dev[s];
  rg->M = Mp;
  rg->rows = M;
  rg->S = p.S;
  rg->lens = dev + (p.lens - slot);
  rg->offs = dev + (p.offs - slot);
  rg->poolrows = dev + (p.pool - slot);
  rg->rowmap = dev + (p.rowmap - slot);
  return 0;
}

static int text_chunk_body(clipx_handle* h, const Call& c, const int32_t* ids_dev, int B, uint16_t* out_f16, float* out_f32) {
  const clipx_model_desc& d = h->desc;
  const ClipWeights& W = h->w;
  const Workspace& ws = h->ws;
  const Tower& X = W.txt;
  hipStream_t st = c.st;
  Ragged rgv{};
  const Ragged* rg = nullptr;
  bool ragged = h->ragged_text && h->pool_last_block && B > GRAPH_MAX_B && X.T <= 128 && X.width / X.heads == 64;
  // A stream that is being captured into a hipGraph: the read-back of device-resident ids needs a synchronisation,
  // and even with the caller's host ids the row map is per-call host data uploaded from a ring slot that later calls overwrite --
  // a replayed graph would upload whatever the slot holds then.  Captured calls run the rectangular tower (same bytes out).
  if (ragged && stream_is_capturing(st)) ragged = false;
  if (ragged) {
    const int32_t* ids_host = c.ids_host;
    if (!ids_host) {  // device-resident ids: one synchronisation of `st` to read them (CLIPX_RAGGED_TEXT=0 keeps the call asynchronous)
      HIPCHK(hipMemcpyAsync(h->ids_back, ids_dev, (size_t)B * X.T * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      ids_host = static_cast<const int32_t*>(h->ids_back.p);
    }
    int rr = ragged_prepare(h, st, ids_host, B, &rgv);
    if (rr) return rr;
    rg = &rgv;
  }
  h->last_text_rows = rg ? rg->M : B * X.T;
  { ProfScope ps(h, st, 3, 0); HIPCHK(launch_text_embed(ids_dev, W.tok_emb, W.txt_pos, nullptr, B, X.T, X.width, d.vocab, st, ws.xn, 1, rg ? rg->rowmap : nullptr, rg ? rg->M : 0)); }
  bool pooled = false;
  int r = run_layers(h, c, X, B, 1, ids_dev, &pooled, rg);
  if (r) return r;
  const void* xf = pooled ? pooled_rows(h, B, X.width) : ws.xn.p;
  { ProfScope ps(h, st, 3, 0); HIPCHK(launch_tail(xf, pooled ? nullptr : ids_dev, X.lnf_w, X.lnf_b, X.proj, out_f16, out_f32, reinterpret_cast<float*>(ws.qkv.p), B, pooled ? 1 : X.T, X.width, d.embed_dim, d.ln_eps, st, 1, c.range_flag)); }
  return 0;
}

int clipx::vision_chunk(clipx_handle* h, const Call& c, const void* pix_dev, int B, int fmt, uint16_t* out_f16, float* out_f32) {
  return run_graphed(h, c.st, GraphCache::Key(c.single_query ? 16 : 0, B, fmt, pix_dev, out_f16, out_f32, c.st), B,
                     [&]() { return vision_chunk_body(h, c, pix_dev, B, fmt, out_f16, out_f32); });
}

int clipx::text_chunk(clipx_handle* h, const Call& c, const int32_t* ids_dev, int B, uint16_t* out_f16, float* out_f32) {
  return run_graphed(h, c.st, GraphCache::Key(c.single_query ? 17 : 1, B, 0, ids_dev, out_f16, out_f32, c.st), B,
                     [&]() { return text_chunk_body(h, c, ids_dev, B, out_f16, out_f32); });
}

// ---------------------------------------------------------------------------------------------
// clipx_profile_*
// ---------------------------------------------------------------------------------------------
extern "C" int clipx_profile_enable(clipx_handle* h, int on) {
  if (!h) return fail(CLIPX_E_ARG, "handle is null");
  std::lock_guard<std::mutex> lk(h->mu);
  Profiler& p = h->prof;
  const int mask = on == 1 ? 15 : ((on >> 1) & 15);  // 1 = every kind; otherwise bit (kind + 1) selects a kind
  if ((mask & 1) && p.chunks.empty()) {
    // the GEMMs' stamp slots: the first chunk is made and filled here, so that no scope has to (ProfScope::next_slot)
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceGetAttribute(&p.clock_khz, hipDeviceAttributeWallClockRate, h->device));
    if (p.clock_khz <= 0) return fail(CLIPX_E_HIP, "hipDeviceAttributeWallClockRate is not positive");
    HIPCHK(p.add_chunk(h->stream));
  }
  p.mask = mask;
  return CLIPX_OK;
}

extern "C" int clipx_profile_events(const clipx_handle* h) { return h ? (int)h->prof.created.size() : 0; }

extern "C" int clipx_profile_get(clipx_handle* h, int kind, int64_t* launches, double* ms, double* flops) {
  if (!h) return fail(CLIPX_E_ARG, "handle is null");
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  Profiler& p = h->prof;
  int64_t n = 0;
  double t = 0.0, f = 0.0;
  std::vector<ProfEvent> keep;
  hipError_t err = hipSuccess;  // the first failure; everything below still consumes every scope and every slot, so that nothing is handed out twice
  // ---- stamp form (all of it is kind 0): wait for the streams the scopes ran on, bring the slots back in one copy per run of ids
  std::vector<std::pair<int, int>> runs;
  if (kind == 0 && p.book.in_use() > 0) {
    std::vector<hipStream_t> streams;
    for (auto& e : p.scopes)
      if (e.stamps && std::find(streams.begin(), streams.end(), e.st) == streams.end()) streams.push_back(e.st);
    for (hipStream_t s : streams) {
      hipError_t r = hipStreamSynchronize(s);
      if (r != hipSuccess && err == hipSuccess) err = r;
    }
    runs = p.book.runs();
    p.host.resize(p.book.capacity());
    for (auto& r : runs) {
      hipError_t c = hipMemcpy(&p.host[r.first], p.slot(r.first), (size_t)r.second * sizeof(StampSlot), hipMemcpyDeviceToHost);
      if (c != hipSuccess && err == hipSuccess) err = c;
    }
  }
  int starved = 0;  // stamp scopes with a slot that still holds its fill value, or with no slot at all: some kernel did not run
  for (auto& e : p.scopes) {
    if (e.kind != kind) {
      keep.push_back(e);
      continue;
    }
    if (e.stamps) {
      unsigned long long ticks = 0;
      bool ok = e.nslots > 0;
      for (int i = 0; i < e.nslots && err == hipSuccess; ++i) {
        unsigned long long t0 = 0, t1 = 0;
        if (stamp_reduce(p.host[e.slot0 + i], &t0, &t1)) ticks += t1 - t0;
        else ok = false;
      }
      if (!ok) ++starved;
      t += (double)ticks / (double)p.clock_khz;  // ticks / kHz = ms
    } else {
      float dt = 0.f;
      hipError_t r = hipEventSynchronize(e.ev[1]);
      if (r == hipSuccess) r = hipEventElapsedTime(&dt, e.ev[0], e.ev[1]);
      if (r != hipSuccess && err == hipSuccess) err = r;
      t += dt;
      for (int i = 0; i < 2; ++i) p.unused.push_back(e.ev[i]);
    }
    f += e.flops;
    ++n;
  }
  p.scopes.swap(keep);
  if (kind == 0 && p.book.in_use() > 0) {  // the slots that were read go back filled
    for (auto& r : runs) {
      hipError_t c = launch_fill_stamps(p.slot(r.first), r.second, h->stream);
      if (c != hipSuccess && err == hipSuccess) err = c;
    }
    hipError_t c = hipStreamSynchronize(h->stream);
    if (c != hipSuccess && err == hipSuccess) err = c;
    p.book.reset();
  }
  const bool out_of_slots = kind == 0 && p.starved;
  if (kind == 0) p.starved = false;
  if (err != hipSuccess) {
    (void)hipGetLastError();
    return fail(CLIPX_E_HIP, std::string("clipx_profile_get: ") + hipGetErrorString(err));
  }
  if (out_of_slots) return fail(CLIPX_E_NOMEM, "clipx_profile_get: the stamp slots ran out and no further chunk could be allocated; some GEMM kernels ran untimed");
  if (starved)
    return fail(CLIPX_E_STATE, "clipx_profile_get: " + std::to_string(starved) + " profiled GEMM scope(s) hold a stamp slot no kernel wrote, or launched no kernel at all (the launch was refused)");
  if (launches) *launches = n;
  if (ms) *ms = t;
  if (flops) *flops = f;
  return CLIPX_OK;
}
