// knnx_api.hip -- host side of the C ABI declared in include/knnx.h (search half of the hot path).
//
// Replaces the faiss Index object the reference holds in ClipResource.image_index
// (clip_retrieval/clip_back.py:781-782) and calls at clip_back.py:362 / clip_filter.py:52,55.
// Owns: the HBM arena of fp16 rows, one HIP stream, per-scan scratch.  No CPU compute path
// exists here on purpose: if HIP is unavailable every entry point fails with KNNX_E_HIP.
// This file: create / add / attach, the flat-family scans and the dispatch between all scans, knnx_search*, the request
// coalescer, reconstruct, statistics.  Range scans and large k: knnx_range.hip; IVF: knnx_ivf.hip; IVF-PQ: knnx_ivfpq.hip;
// the index object and what the files share: knnx_host.h.

#include "knnx_host.h"

int set_dev(const knnx_index* ix) {
  HIPCHK(hipSetDevice(ix->device));
  return 0;
}

int ensure_pin(knnx_index* ix, size_t bytes) {
  HIPCHK(ix->pin.ensure(bytes));
  return 0;
}

int ensure_scratch(knnx_index* ix, int slot, size_t bytes, void** out) {
  knnx_index::Slot& sl = ix->scratch[slot];
  if (sl.bytes < bytes) {
    sl.bytes = 0;
    const size_t want = std::max(bytes, (size_t)1 << 16);
    HIPCHK(malloc_or_reclaim(ix, sl.p, want));
    sl.bytes = want;
  }
  *out = sl.p;
  return 0;
}

int scan_cap(int d, int k) {
  long avail = (long)KNN_LDS_BYTES - (long)d * 128 - KNN_NQ * 8 - 16;
  int cap = (int)(avail / (KNN_NQ * 8));
  cap = std::min(cap, 128);
  cap &= ~1;
  if (cap < k + 16) return -1;
  return cap;
}

extern "C" const char* knnx_last_error(void) { return g_err.c_str(); }
// used by postfilter.hip (same library, other translation unit): set the thread-local message
extern "C" int knnx_set_error(int code, const char* msg) { return fail(code, msg ? msg : ""); }

// an integer switch of the environment (unset or empty: dflt)
static int64_t env_int(const char* name, int64_t dflt) {
  const char* v = getenv(name);
  return (v && v[0]) ? atoll(v) : dflt;
}

extern "C" int knnx_create(int device, int d, int metric, knnx_index** out) {
  if (!out) return fail(KNNX_E_ARG, "out is null");
  *out = nullptr;
  if (metric != KNNX_METRIC_INNER_PRODUCT) return fail(KNNX_E_UNSUPPORTED, "only inner product is implemented");
  if (d <= 0 || d % 256 != 0 || d > 1024)
    return fail(KNNX_E_UNSUPPORTED, "d must be a multiple of 256 and <= 1024 (pad rows with zeros otherwise)");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(KNNX_E_ARG, "no such HIP device");
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return fail(KNNX_E_UNSUPPORTED, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);

  knnx_index* ix = new knnx_index();
  ix->device = device;
  ix->d = d;
  ix->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // every switch of the environment is read here, once
  ix->nt_loads = env_int("KNNX_NT", 0) == 1;
  ix->wide_ok = env_int("KNNX_WIDE", 1) != 0;
  ix->rq_ok = env_int("KNNX_RQ", 1) != 0;
  ix->i8_ok = ix->i8_env_ok = env_int("KNNX_I8", 1) != 0;
  const int64_t pl = env_int("KNNX_I8_PLANES", 0);
  ix->i8_planes_env = (pl == 1 || pl == 2) ? (int)pl : 0;
  ix->i8_dom_off = env_int("KNNX_I8_DOM", 1) == 0;
  ix->i8_budget = std::max<int64_t>(0, env_int("KNNX_I8_MAX_BYTES", 0));
  ix->ivfm_ok = env_int("KNNX_IVF_MULTI", 1) != 0;
  ix->rq_min_rows = env_int("KNNX_RQ_MIN_ROWS", ix->rq_min_rows);
  ix->rq_sample_grid = (int)std::max<int64_t>(0, env_int("KNNX_RQ_SAMPLE_GRID", 0));
  const int64_t gr = env_int("KNNX_GRID", 0);
  if (gr > 0) ix->n_cu = (int)gr;
  hipError_t e = ix->stream.create();
  if (e == hipSuccess) e = ix->flat.alloc(d, (size_t)ix->n_cu);
  if (e == hipSuccess) e = ix->wide.alloc();
  if (e == hipSuccess) e = ix->ev_scratch.create(hipEventDisableTiming);
  if (e != hipSuccess) {
    std::string m = std::string("knnx_create: ") + hipGetErrorString(e);
    knnx_destroy(ix);
    return fail(KNNX_E_HIP, m);
  }
  *out = ix;
  return KNNX_OK;
}

// (every buffer, the stream and the events are owned by their members: knnx_host.h)
extern "C" void knnx_destroy(knnx_index* ix) {
  if (!ix) return;
  hipSetDevice(ix->device);
  if (ix->stream) hipStreamSynchronize(ix->stream);
  {  // a translation of ids still running on its own stream (knnx_ivf_map_ids) finishes first
    std::lock_guard<std::mutex> lk(ix->ido.mu);
    if (ix->ido.stream) hipStreamSynchronize(ix->ido.stream);
  }
  if (ix->cent) knnx_destroy(ix->cent);
  hipSetDevice(ix->device);
  delete ix;
}

extern "C" int64_t knnx_ntotal(const knnx_index* ix) { return ix ? ix->ntotal : 0; }
extern "C" int knnx_dim(const knnx_index* ix) { return ix ? ix->d : 0; }

// faiss Index.reset(): forget the rows, keep the arena (the per-request dedup index of clip_back.py:290-294 is rebuilt from
// the <= k result vectors of every query; allocating a fresh index per request would cost more than the search)
extern "C" int knnx_reset(knnx_index* ix) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (ix->pq.m) return fail(KNNX_E_STATE, "reset of an IVF-PQ index is not supported (destroy it instead)");
  if (ix->sq.on) return fail(KNNX_E_STATE, "reset of an IVF-SQ8 index is not supported (destroy it instead)");
  if (ix->ivf_nlist || ix->ivfb.nlist) return fail(KNNX_E_STATE, "reset of an IVF index is not supported (destroy it instead)");
  if (set_dev(ix)) return KNNX_E_HIP;
  HIPCHK(hipStreamSynchronize(ix->stream));
  ix->ntotal = 0;
  ix->i8.valid = false;
  ix->i8.nrows = 0;
  ix->i8_ok = ix->i8_env_ok;  // a copy that was given up for lack of memory may be tried again for the new rows; KNNX_I8=0 still rules
  HIPCHK(hipMemsetAsync(ix->flat.maxnorm, 0, sizeof(int), ix->stream));
  return KNNX_OK;
}

extern "C" int knnx_set_id_base(knnx_index* ix, int64_t id_base) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  ix->id_base = id_base;
  return KNNX_OK;
}

static int grow(knnx_index* ix, int64_t need_rows) {
  if (need_rows <= ix->capacity) return 0;
  if (ix->rows.borrowed) return fail(KNNX_E_STATE, "index borrows caller memory; cannot grow");
  if (need_rows > (int64_t)0xffffffffll) return fail(KNNX_E_UNSUPPORTED, "more than 2^32 rows per device");
  DevBuf<_Float16> nr;
  if (nr.alloc((size_t)need_rows * ix->d) != hipSuccess) {
    (void)hipGetLastError();
    // the int8 copy is an accelerator, not data: give its memory back and try once more
    ix->i8.release();
    HIPCHK(nr.alloc((size_t)need_rows * ix->d));
  }
  if (ix->rows && ix->ntotal > 0) {
    hipError_t e = hipMemcpyAsync(nr, ix->rows, (size_t)ix->ntotal * ix->d * sizeof(_Float16),
                                  hipMemcpyDeviceToDevice, ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess) return fail(KNNX_E_HIP, std::string("grow copy: ") + hipGetErrorString(e));
  }
  ix->rows = std::move(nr);
  ix->capacity = need_rows;
  return 0;
}

extern "C" int knnx_reserve(knnx_index* ix, int64_t n_rows) {
  if (!ix || n_rows < 0) return fail(KNNX_E_ARG, "bad reserve");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (ix->pq.m) return fail(KNNX_E_STATE, "reserve on an IVF-PQ index (its arena is sized by knnx_ivf_begin)");
  if (ix->sq.on) return fail(KNNX_E_STATE, "reserve on an IVF-SQ8 index (its arena is sized by knnx_ivf_begin)");
  return grow(ix, n_rows);
}

static int add_common(knnx_index* ix, const void* rows, int64_t n, bool is_f32) {
  if (!ix || (!rows && n > 0) || n < 0) return fail(KNNX_E_ARG, "bad add arguments");
  if (n == 0) return KNNX_OK;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (ix->rows.borrowed) return fail(KNNX_E_STATE, "add() on an index that borrows device rows");
  if (ix->pq.m) return fail(KNNX_E_STATE, "add() on an IVF-PQ index (rows are encoded by knnx_ivf_begin / knnx_ivf_add_assigned / knnx_ivf_end)");
  if (ix->sq.on) return fail(KNNX_E_STATE, "add() on an IVF-SQ8 index (rows are encoded by knnx_ivf_begin / knnx_ivf_add_assigned / knnx_ivf_end)");
  if (ix->ivf_nlist) return fail(KNNX_E_STATE, "add() after knnx_ivf_set_lists (rebuild the index instead)");
  if (ix->ntotal + n > ix->capacity) {
    int64_t want = std::max<int64_t>(ix->ntotal + n, ix->capacity + ix->capacity / 2);
    int r = grow(ix, want);
    if (r) return r;
  }
  const size_t esz = is_f32 ? 4 : 2;
  const int64_t chunk_rows = std::max<int64_t>(1, (int64_t)(64u << 20) / (int64_t)(ix->d * esz));
  int r = ensure_pin(ix, (size_t)chunk_rows * ix->d * esz);
  if (r) return r;
  DevBuf<float> tmp32;
  if (is_f32) HIPCHK(tmp32.alloc((size_t)chunk_rows * ix->d));
  for (int64_t o = 0; o < n; o += chunk_rows) {
    const int64_t m = std::min(chunk_rows, n - o);
    const size_t bytes = (size_t)m * ix->d * esz;
    memcpy(ix->pin.p, (const char*)rows + (size_t)o * ix->d * esz, bytes);
    _Float16* dst = ix->rows + (size_t)(ix->ntotal + o) * ix->d;
    hipError_t e;
    if (is_f32) {
      e = hipMemcpyAsync(tmp32, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->stream);
      if (e == hipSuccess) e = launch_f32_to_f16(tmp32, dst, m * ix->d, ix->stream);
    } else {
      e = hipMemcpyAsync(dst, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->stream);
    }
    if (e == hipSuccess) e = launch_maxnorm(dst, m, ix->d, ix->flat.maxnorm, ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess) return fail(KNNX_E_HIP, std::string("add copy: ") + hipGetErrorString(e));
  }
  ix->ntotal += n;
  ix->i8.valid = false;  // (the rows quantised so far stay: i8_ensure quantises [i8_nrows, ntotal) only)
  return KNNX_OK;
}

extern "C" int knnx_add_f16(knnx_index* ix, const uint16_t* rows, int64_t n) { return add_common(ix, rows, n, false); }
extern "C" int knnx_add_f32(knnx_index* ix, const float* rows, int64_t n) { return add_common(ix, rows, n, true); }

extern "C" int knnx_attach_device_f16(knnx_index* ix, const void* dev_rows, int64_t n) {
  if (!ix || !dev_rows || n < 0) return fail(KNNX_E_ARG, "bad attach arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (ix->pq.m) return fail(KNNX_E_STATE, "attach on an IVF-PQ index");
  if (ix->sq.on) return fail(KNNX_E_STATE, "attach on an IVF-SQ8 index");
  if (ix->rows && !ix->rows.borrowed) return fail(KNNX_E_STATE, "index already owns rows");
  if (n > (int64_t)0xffffffffll) return fail(KNNX_E_UNSUPPORTED, "more than 2^32 rows per device");
  ix->rows.borrow(dev_rows);
  ix->capacity = n;
  ix->ntotal = n;
  ix->i8.valid = false;
  ix->i8.nrows = 0;
  if (set_dev(ix)) return KNNX_E_HIP;
  HIPCHK(hipMemsetAsync(ix->flat.maxnorm, 0, sizeof(int), ix->stream));
  HIPCHK(launch_maxnorm(ix->rows, n, ix->d, ix->flat.maxnorm, ix->stream));
  HIPCHK(hipStreamSynchronize(ix->stream));
  return KNNX_OK;
}

extern "C" int knnx_synth_fill(knnx_index* ix, int64_t n, uint64_t seed) {
  if (!ix || n < 0) return fail(KNNX_E_ARG, "bad synth arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (ix->pq.m) return fail(KNNX_E_STATE, "synth_fill on an IVF-PQ index");
  if (ix->sq.on) return fail(KNNX_E_STATE, "synth_fill on an IVF-SQ8 index");
  if (!ix->rows.borrowed) {
    int r = grow(ix, n);
    if (r) return r;
  } else if (n > ix->capacity) {
    return fail(KNNX_E_NOMEM, "attached arena is smaller than n");
  }
  HIPCHK(launch_synth(ix->rows, 0, n, ix->d, seed, ix->stream));
  HIPCHK(hipMemsetAsync(ix->flat.maxnorm, 0, sizeof(int), ix->stream));
  HIPCHK(launch_maxnorm(ix->rows, n, ix->d, ix->flat.maxnorm, ix->stream));
  HIPCHK(hipStreamSynchronize(ix->stream));
  ix->ntotal = n;
  ix->i8.valid = false;
  ix->i8.nrows = 0;
  return KNNX_OK;
}

// one scan of <= KNN_NQ queries already in HBM; results land in D_out/I_out (device, [nq, k])
int scan_topk(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st, const unsigned* gate) {
  const int cap = scan_cap(ix->d, k);
  if (cap < 0) return fail(KNNX_E_UNSUPPORTED, "k too large for the LDS queues at this d");
  if (ix->ivf_nlist) {
    int r = ivf_build_worklist(ix, q_dev, nq, st, gate);
    if (r) return r;
    ix->ivfm_last_blk = 0;
  }
  HIPCHK(launch_prep(q_dev, nq, ix->d, ix->flat.qfrag, ix->flat.thr_g, nullptr, 0, gate, st));
  ScanArgs a{};
  a.gate = gate;
  a.X = ix->rows;
  a.N = ix->ivf_nlist ? ix->capacity : ix->ntotal;
  a.d = ix->d;
  a.qfrag = ix->flat.qfrag;
  a.nq = nq;
  a.k = k;
  a.cap = cap;
  a.grid = ix->n_cu;
  a.mode = 0;
  a.nt = ix->nt_loads;
  a.thr_g = ix->flat.thr_g;
  a.part_s = ix->flat.part_s;
  a.part_i = ix->flat.part_i;
  a.part_n = ix->flat.part_n;
  a.work = ix->ivf_nlist ? ix->ivf1.work : nullptr;
  a.nwork = ix->ivf1.nwork;
  const bool prof = ix->prof.on && !gate;  // gated fallback scans normally exit at once: not a scan launch worth timing
  HIPCHK(ix->prof.begin(prof, st));
  HIPCHK(launch_scan(a, st));
  HIPCHK(ix->prof.end(prof, st));
  HIPCHK(launch_merge_u32(ix->flat.part_s, ix->flat.part_i, ix->flat.part_n, ix->n_cu, KNN_NQ, k, nq, k, ix->id_base,
                          ix->ivf_nlist ? ix->ivf.idmap : nullptr, D_out, I_out, gate, st));
  return 0;
}

// the exact scan of every 32-query group of a proof-based scan, gated on the device by gate[g] -- or (ix->defer_fb) left to the host
// entry point, which reads the gates back: see knnx_index::defer_fb
static int fallback_groups(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st, int kind) {
  unsigned* need = kind == 1 ? ix->rq.need : ix->wide.need;
  unsigned* gate = kind == 1 ? ix->rq.gate : ix->wide.gate;
  if (ix->defer_fb) {
    ix->defer_kind = kind;
    ix->defer_nq = nq;
    return 0;
  }
  for (int g = 0; g * KNN_NQ < nq; ++g) {
    const int q0 = g * KNN_NQ, n = std::min(KNN_NQ, nq - q0);
    int r = scan_topk(ix, q_dev + (size_t)q0 * ix->d, n, k, ix->wide.Dfb, ix->wide.Ifb, st, gate + g);
    if (r) return r;
    HIPCHK(launch_select(need, q0, n, k, ix->wide.Dfb, ix->wide.Ifb, D_out, I_out, st));
  }
  return 0;
}

// LDS capacity of the 64-queue wide scan at this d
static int wide_cap(int d) {
  long avail = (long)KNN_LDS_BYTES - (long)d * 128 - KNN_NQ_MAX * 8 - 16;
  int cap = (int)(avail / (KNN_NQ_MAX * 8));
  cap = std::min(cap, 128) & ~1;
  return cap >= KNN_WIDE_KW + 16 ? cap : -1;
}
static bool wide_usable(const knnx_index* ix, int nq, int k) {
  return ix->wide_ok && !ix->ivf_nlist && nq > KNN_NQ && k <= KNN_WIDE_MAX_K && wide_cap(ix->d) > 0;
}

// one WIDE scan of 33..64 queries: approximate top-64 by fp16-hi score in ONE pass over HBM, exact re-scoring of the 64
// candidates, proof of exactness per query; a query whose proof fails gets the exact 32-query scan of its half, which
// is launched unconditionally but exits at once unless its gate was set by the proof kernel (no host round trip).
static int scan_topk_wide(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st) {
  const int cap = wide_cap(ix->d);
  HIPCHK(launch_prep(q_dev, nq, ix->d, ix->flat.qfrag, ix->flat.thr_g, nullptr, 1, nullptr, st));
  ScanArgs a{};
  a.X = ix->rows;
  a.N = ix->ntotal;
  a.d = ix->d;
  a.qfrag = ix->flat.qfrag;
  a.nq = nq;
  a.k = KNN_WIDE_KW;
  a.cap = cap;
  a.grid = ix->n_cu;
  a.mode = 0;
  a.wide = 1;
  a.thr_g = ix->flat.thr_g;
  a.part_s = ix->flat.part_s;
  a.part_i = ix->flat.part_i;
  a.part_n = ix->flat.part_n;
  HIPCHK(ix->prof.begin(ix->prof.on, st));
  HIPCHK(launch_scan(a, st));
  HIPCHK(ix->prof.end(ix->prof.on, st));
  HIPCHK(launch_merge_u32(ix->flat.part_s, ix->flat.part_i, ix->flat.part_n, ix->n_cu, KNN_NQ_MAX, KNN_WIDE_KW, nq, KNN_WIDE_KW, 0, nullptr,
                          ix->wide.approx, ix->wide.cand, nullptr, st));
  HIPCHK(launch_rescore(ix->rows, ix->d, q_dev, ix->wide.cand, ix->wide.approx, nq, KNN_WIDE_KW, k, ix->id_base, ix->flat.maxnorm,
                        D_out, I_out, ix->wide.need, ix->wide.gate, ix->flat.stats, st));
  return fallback_groups(ix, q_dev, nq, k, D_out, I_out, st, 2);
}


// ---- scratch guard: call at the start / end of every launch sequence that uses the handle's scratch (caller holds mu)
int scratch_acquire(knnx_index* ix, hipStream_t st) {
  if (ix->ev_valid) HIPCHK(hipStreamWaitEvent(st, ix->ev_scratch, 0));
  return 0;
}
int scratch_release(knnx_index* ix, hipStream_t st) {
  HIPCHK(hipEventRecord(ix->ev_scratch, st));
  ix->ev_valid = true;
  return 0;
}

// ---- RQ scan: up to rq_queries_per_pass(d) queries in ONE pass over HBM (see knn_rq_kernels.hip)
static bool rq_usable(const knnx_index* ix, int nq, int k) {
  return ix->rq_ok && ix->wide_ok && !ix->ivf_nlist && nq > KNN_NQ_MAX && k <= KNN_WIDE_MAX_K && rq_queries_per_pass(ix->d) > 0 &&
         ix->ntotal >= ix->rq_min_rows && scan_cap(ix->d, KNN_WIDE_KW) > 0;
}
static int rq_alloc(knnx_index* ix) {
  HIPCHK(ix->rq.alloc(ix->d));
  return 0;
}
// thresholds of a register-stationary pass: the 64-query scan over every S-th tile, S = min(stride_cap, tiles / 4096); the J-th best
// sample score of query q -> ix->rq.samp[q * KNN_WIDE_KW + J - 1] (knn_kernels.h: KNN_RQ_STRIDE).  Returns S and J through the pointers.
static int rq_sample_pass(knnx_index* ix, const float* q_dev, int nq, int k, int stride_cap, hipStream_t st, int* tstride_out, int* J_out,
                          bool* wide_samp_out) {
  const int d = ix->d;
  const int64_t ntiles = (ix->ntotal + 31) / 32;
  const int tstride = (int)std::max<int64_t>(1, std::min<int64_t>(stride_cap, ntiles / 4096));
  // (the 64-query wide scan where its LDS queues fit, d <= 768; at d = 1024 the exact 32-query scan, whose scores are exact
  // rather than fp16-hi: the threshold then gets a slack of a few eps so that the sample rows themselves still reach it)
  const bool wide_samp = wide_cap(d) > 0;
  const int gsz = wide_samp ? KNN_NQ_MAX : KNN_NQ;
  // The sample scans cost a fixed ~0.45 ms each whatever their grid (cold candidate queues: every workgroup floods and prunes
  // its queues a few times before its thresholds bite; 256 -> 64 workgroups: same time, tools/rq_sample_grid.py), and one of
  // them needs a whole CU's LDS per workgroup.  So the groups of a batch run side by side as blocks of ONE launch
  // (knn_scan_kernel, nblk: workgroup g serves group g % ngroups), each on its share of the CUs: 4 x (prep + scan + merge) in
  // the time of one.  (Round 6; a stream per group lost to it -- four streams only run side by side while the runtime has four
  // hardware queues to give them, profiles/r06r_knn_b256_timeline.log.)
  const int ngroups = (nq + gsz - 1) / gsz;
  const int jfull = std::min(KNN_WIDE_KW, k + KNN_RQ_MARGIN);
  const int J = tstride <= 128 ? jfull : std::max(6, std::min(jfull, (jfull * 128 + tstride - 1) / tstride));
  *tstride_out = tstride;
  *J_out = J;
  *wide_samp_out = wide_samp;
  if (ngroups > 1 && ngroups <= KNN_RQ_MAX / KNN_NQ && ix->n_cu >= ngroups) {
    const int grid = std::max(1, ix->n_cu / ngroups) * ngroups;
    // only the J-th best sample score of a query is used: the queues keep J entries (>= 8), not 64 -- their thresholds rise sooner and
    // the cold-queue pruning that makes up most of this scan's time (see above) ends sooner
    const int ks = std::min(KNN_WIDE_KW, std::max(8, J));
    if (grid <= ix->n_cu) {
      HIPCHK(launch_prep_blocks(q_dev, nq, d, ix->rq.m_qfrag, ix->rq.m_thr, nullptr, st, wide_samp ? 1 : 0));
      ScanArgs a{};
      a.X = ix->rows;
      a.N = ix->ntotal;
      a.d = d;
      a.qfrag = ix->rq.m_qfrag;
      a.nq = nq;
      a.k = ks;
      a.cap = wide_samp ? wide_cap(d) : scan_cap(d, KNN_WIDE_KW);
      a.grid = grid;
      a.mode = 0;
      a.wide = wide_samp ? 1 : 0;
      a.tstride = tstride;
      a.thr_g = ix->rq.m_thr;
      a.part_s = ix->flat.part_s;
      a.part_i = ix->flat.part_i;
      a.part_n = ix->flat.part_n;
      a.nblk = ngroups;
      HIPCHK(launch_scan(a, st));
      HIPCHK(launch_merge_u32(ix->flat.part_s, ix->flat.part_i, ix->flat.part_n, grid / ngroups, gsz, ks, nq, KNN_WIDE_KW, 0, nullptr, ix->rq.samp,
                              ix->rq.samp_i, nullptr, st, gsz));  // (rows of 64 with the entries past ks padded: the preps read entry J - 1)
      return 0;
    }
  }
  // a single group, or KNNX_GRID leaves fewer workgroups than groups: one group after the other on the caller's stream
  const int sgrid = std::max(1, std::min(ix->n_cu, ix->rq_sample_grid > 0 ? ix->rq_sample_grid : ix->n_cu));
  for (int g = 0; g * gsz < nq; ++g) {
    const int q0 = g * gsz, n = std::min(gsz, nq - q0);
    HIPCHK(launch_prep(q_dev + (size_t)q0 * d, n, d, ix->flat.qfrag, ix->flat.thr_g, nullptr, wide_samp ? 1 : 0, nullptr, st));
    ScanArgs a{};
    a.X = ix->rows;
    a.N = ix->ntotal;
    a.d = d;
    a.qfrag = ix->flat.qfrag;
    a.nq = n;
    a.k = KNN_WIDE_KW;
    a.cap = wide_samp ? wide_cap(d) : scan_cap(d, KNN_WIDE_KW);
    a.grid = sgrid;
    a.mode = 0;
    a.wide = wide_samp ? 1 : 0;
    a.tstride = tstride;
    a.thr_g = ix->flat.thr_g;
    a.part_s = ix->flat.part_s;
    a.part_i = ix->flat.part_i;
    a.part_n = ix->flat.part_n;
    HIPCHK(launch_scan(a, st));
    HIPCHK(launch_merge_u32(ix->flat.part_s, ix->flat.part_i, ix->flat.part_n, sgrid, gsz, KNN_WIDE_KW, n, KNN_WIDE_KW, 0, nullptr,
                            ix->rq.samp + (size_t)q0 * KNN_WIDE_KW, ix->rq.samp_i + (size_t)q0 * KNN_WIDE_KW, nullptr, st));
  }
  return 0;
}

static int scan_topk_rq(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st) {
  int r = rq_alloc(ix);
  if (r) return r;
  const int d = ix->d;
  // 1. thresholds: the sample pass
  int tstride = 1, J = 1;
  bool wide_samp = false;
  r = rq_sample_pass(ix, q_dev, nq, k, KNN_RQ_STRIDE, st, &tstride, &J, &wide_samp);
  if (r) return r;
  HIPCHK(launch_rq_prep(q_dev, nq, d, ix->rq.qfrag, ix->rq.samp, KNN_WIDE_KW, J, wide_samp ? 0.f : 1e-3f, ix->rq.thr, ix->rq.cnt,
                        ix->rq.lost, st));
  // 2. the pass over the whole index
  HIPCHK(ix->prof.begin(ix->prof.on, st));
  HIPCHK(launch_rq_scan(ix->rows, ix->ntotal, d, nq, ix->rq.qfrag, ix->rq.thr, ix->rq.cnt, KNN_RQ_CAP, ix->rq.hit_s, ix->rq.hit_r,
                        ix->rq.lost, nullptr, ix->n_cu, st));
  HIPCHK(ix->prof.end(ix->prof.on, st));
  // 3. exact scores of the hits, exact top-k among them, proof
  HIPCHK(launch_rq_rescore(ix->rows, d, q_dev, nq, ix->rq.cnt, KNN_RQ_CAP, ix->rq.hit_s, ix->rq.hit_r, ix->rq.cntc, st));
  HIPCHK(launch_merge_u32(ix->rq.hit_s, ix->rq.hit_r, ix->rq.cntc, 1, nq, (int)KNN_RQ_CAP, nq, k, ix->id_base, nullptr, D_out, I_out,
                          nullptr, st));
  HIPCHK(launch_rq_proof(q_dev, nq, d, k, D_out, ix->rq.thr, ix->rq.cnt, KNN_RQ_CAP, ix->rq.lost, ix->flat.maxnorm, ix->rq.need,
                         ix->rq.gate, ix->flat.stats, st));
  // 4. unproven queries: the exact scan of their 32-query group, gated on the device (or left to the host entry point)
  return fallback_groups(ix, q_dev, nq, k, D_out, I_out, st, 1);
}

// ---- int8 first stage (knn_rq_kernels.hip, "int8 first stage"): 1 .. 256 queries in ONE pass over the int8 copy of the rows
static bool i8_usable(const knnx_index* ix, int nq, int k) {
  return ix->i8_ok && ix->rq_ok && ix->wide_ok && !ix->ivf_nlist && nq >= 1 && k <= KNN_WIDE_MAX_K && i8_supported(ix->d) &&
         ix->ntotal >= ix->rq_min_rows && scan_cap(ix->d, KNN_WIDE_KW) > 0;
}
// allocate (first use) and build (first use, and after the rows changed) the int8 copy; 1: ready, 0: not available (the caller takes
// another path; out of memory turns the feature off for this index), < 0: error.
// The copy may be PARTIAL (round 5): when ntotal * d bytes do not fit next to the fp16 rows -- BASELINE's headline shard, 125 M x 768 =
// 192 GB of fp16 on a 288 GB part, leaves room for ~80 M rows of int8 -- or KNNX_I8_MAX_BYTES caps it, rows [0, i8_nrows) get the int8
// first stage and the rows behind them are scanned by the fp16 register-stationary pass into the same hit lists (scan_topk_i8).
static int i8_ensure(knnx_index* ix, hipStream_t st) {
  if (ix->i8.valid) return 1;
  auto give_up = [&]() {
    (void)hipGetLastError();
    ix->i8_ok = 0;
    ix->i8.release();
    return 0;
  };
  if (ix->i8q.alloc(ix->d) != hipSuccess) return give_up();
  // everything else the flat scans allocate lazily comes FIRST, so that a partial copy is sized around it, not the other way round
  int r = rq_alloc(ix);
  if (r) return r;
  const auto tiles32 = [](int64_t rows) { return (rows + 31) & ~(int64_t)31; };
  if (ix->i8.cap_rows < ix->ntotal) {
    // (an owned index grows by halves: follow its capacity, so that a stream of add() calls does not reallocate every time)
    int64_t want = tiles32(std::max(ix->ntotal, ix->rows.borrowed ? ix->ntotal : ix->capacity));
    if (ix->i8_budget > 0) want = std::min(want, (ix->i8_budget / ix->d) & ~(int64_t)31);
    DevBuf<int8_t> nr;
    if (want > ix->i8.cap_rows && nr.alloc((size_t)want * ix->d) != hipSuccess) {
      (void)hipGetLastError();
      // what is free, less a reserve for the pools that are sized per request (range scans: up to 4 GiB, large-k scratch, reconstruct)
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) != hipSuccess) return give_up();
      const size_t have = (size_t)ix->i8.cap_rows * ix->d;  // the old image is released below: its bytes count as free
      const size_t reserve = (size_t)8 << 30;
      want = fr + have > reserve ? (int64_t)(((fr + have - reserve) / (size_t)ix->d) & ~(size_t)31) : 0;
      if (want > tiles32(ix->ntotal)) want = tiles32(ix->ntotal);
      // a copy of less than a quarter of the rows saves under an eighth of the pass: not worth the memory
      if (want < ix->ntotal / 4 || want <= ix->i8.cap_rows) {
        if (want <= ix->i8.cap_rows && ix->i8.cap_rows >= ix->ntotal / 4) want = 0;  // keep the image that exists
        else return give_up();
      }
      if (want > 0) {
        // the old image has to go first (its bytes are part of the estimate); what it held is quantised again below
        ix->i8.release();
        if (nr.alloc((size_t)want * ix->d) != hipSuccess) return give_up();
      }
    }
    if (nr) {
      if (ix->i8.rows && ix->i8.nrows > 0) {
        // whole tiles of the old image carry over (tile-ordered: a prefix of tiles is a prefix of bytes)
        const int64_t keep = std::min(ix->i8.nrows & ~(int64_t)31, want);
        hipError_t e = keep > 0 ? hipMemcpyAsync(nr, ix->i8.rows, (size_t)keep * ix->d, hipMemcpyDeviceToDevice, st) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(KNNX_E_HIP, std::string("int8 copy: ") + hipGetErrorString(e));
        ix->i8.nrows = keep;
      }
      ix->i8.rows = std::move(nr);
      ix->i8.cap_rows = want;
    }
  }
  const int64_t n8 = std::min(ix->ntotal, ix->i8.cap_rows);  // rows the image will hold
  if (n8 < ix->ntotal / 4) return give_up();
  if (ix->i8.nrows > 0 && ix->i8.nrows <= n8 && ix->ntotal < 2 * ix->i8.scale_rows) {
    // rows were appended: quantise the new ones with the scales that exist (values beyond them clamp; A and B grow with what is stored)
    if (ix->i8.nrows < n8)
      HIPCHK(launch_i8_quant(ix->rows, n8, ix->i8.nrows, n8, ix->d, ix->i8q.colscale, ix->i8.dom, ix->i8.rows, ix->i8q.ab, st));
  } else {
    HIPCHK(launch_i8_scales(ix->rows, ix->ntotal, ix->d, ix->i8q.colmax, ix->i8q.colscale, ix->i8q.ab, st));
    ix->i8.scale_rows = ix->ntotal;
    // The form of the first stage is part of the build (a readback of d floats: the build is about to move the whole index).  A query's
    // u = q * c has ONE scale, so a few columns much larger than the rest (CLIP embeddings have them) leave the others' components in
    // the rounding error.  Columns whose scale is more than 3 x the median one are "dominant":
    //   1 .. 4 of them: they move to bytes 0..3 of each row of the image and the scan handles them with 14-bit query digits (I8Dom) --
    //                   one plane, 256 queries per pass
    //   more:           two int8 planes per query (twice the MFMAs, 128 queries per pass)
    std::vector<float> cs((size_t)ix->d);
    HIPCHK(hipMemcpyAsync(cs.data(), ix->i8q.colscale, (size_t)ix->d * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<float> sorted(cs);
    std::nth_element(sorted.begin(), sorted.begin() + ix->d / 2, sorted.end());
    const float cmed = sorted[(size_t)ix->d / 2];
    std::vector<int> big;
    for (int c = 0; c < ix->d; ++c)
      if (cs[(size_t)c] > 3.f * cmed) big.push_back(c);
    ix->i8.dom = I8Dom();
    if (ix->i8_planes_env) {
      ix->i8.planes = ix->i8_planes_env;
    } else if (!big.empty() && big.size() <= 4 && !ix->i8_dom_off) {
      ix->i8.planes = 1;
      // the permutation that brings them to positions 0 .. n - 1: a swap per dominant column
      std::vector<int> perm((size_t)ix->d);
      for (int c = 0; c < ix->d; ++c) perm[(size_t)c] = c;
      for (size_t j = 0; j < big.size(); ++j) {
        const size_t at = (size_t)(std::find(perm.begin(), perm.end(), big[j]) - perm.begin());
        std::swap(perm[j], perm[at]);
      }
      ix->i8.dom.n = (int)big.size();
      for (int c = 0; c < ix->d; ++c)
        if (perm[(size_t)c] != c) {
          ix->i8.dom.pos[ix->i8.dom.nfix] = c;
          ix->i8.dom.src[ix->i8.dom.nfix] = perm[(size_t)c];
          ++ix->i8.dom.nfix;  // (at most two positions per swap: 8)
        }
    } else {
      ix->i8.planes = big.empty() ? 1 : 2;
    }
    HIPCHK(launch_i8_quant(ix->rows, n8, 0, n8, ix->d, ix->i8q.colscale, ix->i8.dom, ix->i8.rows, ix->i8q.ab, st));
  }
  ix->i8.nrows = n8;
  ix->i8.valid = true;
  return 1;
}
static int scan_topk_i8(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st) {
  int r = rq_alloc(ix);
  if (r) return r;
  const int d = ix->d;
  const int64_t n8 = ix->i8.nrows;          // rows [0, n8) have an int8 image ...
  const int64_t nrest = ix->ntotal - n8;    // ... the rows behind them are scanned in fp16 (partial copy, i8_ensure)
  // 1. thresholds: the exact sample pass (denser than the fp16 path's: the int8 bound widens the admission band, a tighter
  // threshold buys the hits back)
  int tstride = 1, J = 1;
  bool wide_samp = false;
  const int64_t ntiles = (ix->ntotal + 31) / 32;
  // Up to 64 queries: ONE exact sample pass over every 32nd tile (one 64-query scan, ~0.8 ms at 100 M rows).  More: four such scans
  // side by side cost ~3 ms of a 25 ms batch, so the threshold comes in two levels -- the coarse exact sample of the fp16 path (every
  // 763rd tile), then an int8 pass over every 32nd tile with THAT threshold (one pass for all the queries: 2.4 GB), whose hits are
  // re-scored exactly; their J-th best score is the threshold of the pass over everything.
  const bool two_level = nq > KNN_NQ_MAX && ntiles >= (int64_t)4096 * KNN_I8_STRIDE;
  r = rq_sample_pass(ix, q_dev, nq, k, two_level ? KNN_RQ_STRIDE : KNN_I8_STRIDE, st, &tstride, &J, &wide_samp);
  if (r) return r;
  float* thr_rest = nrest > 0 ? ix->rq.thr : nullptr;
  const int8_t* qdom = ix->i8.dom.n > 0 ? ix->i8q.qdom : nullptr;
  HIPCHK(launch_i8_prep(q_dev, nq, d, ix->i8q.colscale, ix->i8.dom, ix->i8q.ab, ix->flat.maxnorm, ix->rq.samp, KNN_WIDE_KW, J, ix->i8.planes, 0,
                        ix->i8q.qfrag, ix->i8q.qdom, ix->i8q.thr, ix->i8q.lb, thr_rest, ix->rq.cnt, ix->rq.lost, st));
  if (two_level) {
    HIPCHK(launch_rq8_scan(ix->i8.rows, n8, d, nq, ix->i8.planes, ix->i8q.qfrag, qdom, ix->i8q.thr, ix->rq.cnt, KNN_I8_CAP, ix->i8q.hit_s,
                           ix->i8q.hit_r, ix->rq.lost, ix->n_cu, KNN_I8_STRIDE, st));
    HIPCHK(launch_rq_rescore(ix->rows, d, q_dev, nq, ix->rq.cnt, KNN_I8_CAP, ix->i8q.hit_s, ix->i8q.hit_r, ix->rq.cntc, st));
    // the exact top-64 of the sampled hits, where the sample passes put theirs: the refining prep reads its J-th entry
    HIPCHK(launch_merge_u32(ix->i8q.hit_s, ix->i8q.hit_r, ix->rq.cntc, 1, nq, (int)KNN_I8_CAP, nq, KNN_WIDE_KW, 0, nullptr, ix->rq.samp,
                            ix->rq.samp_i, nullptr, st));
    const int J2 = std::min(KNN_WIDE_KW, k + KNN_RQ_MARGIN);
    HIPCHK(launch_i8_prep(q_dev, nq, d, ix->i8q.colscale, ix->i8.dom, ix->i8q.ab, ix->flat.maxnorm, ix->rq.samp, KNN_WIDE_KW, J2, ix->i8.planes, 1,
                          ix->i8q.qfrag, ix->i8q.qdom, ix->i8q.thr, ix->i8q.lb, thr_rest, ix->rq.cnt, ix->rq.lost, st));
  }
  // 2. the pass over the int8 rows
  HIPCHK(ix->prof.begin(ix->prof.on, st));
  HIPCHK(launch_rq8_scan(ix->i8.rows, n8, d, nq, ix->i8.planes, ix->i8q.qfrag, qdom, ix->i8q.thr, ix->rq.cnt, KNN_I8_CAP, ix->i8q.hit_s, ix->i8q.hit_r,
                         ix->rq.lost, ix->n_cu, 1, st));
  // 2b. the rows without an int8 image: the fp16 register-stationary pass, admission threshold T - eps_hi (knn_i8_prep_kernel), into
  // the SAME hit lists (global row = n8 + row of the slice); the lower bound T of the proof covers both parts
  if (nrest > 0) {
    const int per = rq_queries_per_pass(d);
    for (int q0 = 0; q0 < nq; q0 += per) {
      const int n = std::min(per, nq - q0);
      HIPCHK(launch_rq_prep(q_dev + (size_t)q0 * d, n, d, ix->rq.qfrag, nullptr, 0, 0, 0.f, nullptr, nullptr, nullptr, st));  // fragments only
      HIPCHK(launch_rq_scan(ix->rows + (size_t)n8 * d, nrest, d, n, ix->rq.qfrag, ix->rq.thr + q0, ix->rq.cnt + q0, KNN_I8_CAP,
                            ix->i8q.hit_s + (size_t)q0 * KNN_I8_CAP, ix->i8q.hit_r + (size_t)q0 * KNN_I8_CAP, ix->rq.lost + q0, nullptr,
                            ix->n_cu, st, (uint32_t)n8));
    }
    ix->i8.rest_served += (unsigned long long)nq;
  }
  HIPCHK(ix->prof.end(ix->prof.on, st));
  // 3. exact scores of the hits (fp16 rows), exact top-k among them, proof
  HIPCHK(launch_rq_rescore(ix->rows, d, q_dev, nq, ix->rq.cnt, KNN_I8_CAP, ix->i8q.hit_s, ix->i8q.hit_r, ix->rq.cntc, st));
  HIPCHK(launch_merge_u32(ix->i8q.hit_s, ix->i8q.hit_r, ix->rq.cntc, 1, nq, (int)KNN_I8_CAP, nq, k, ix->id_base, nullptr, D_out, I_out,
                          nullptr, st));
  HIPCHK(launch_i8_proof(nq, k, D_out, ix->i8q.lb, ix->rq.cnt, KNN_I8_CAP, ix->rq.lost, ix->rq.need, ix->rq.gate, ix->flat.stats, st));
  // 4. unproven queries (a hit list overflowed): the exact scan of their 32-query group, gated on the device (or left to the host
  // entry point)
  ix->i8.served += (unsigned long long)nq;
  return fallback_groups(ix, q_dev, nq, k, D_out, I_out, st, 1);
}

// ---- the dispatch policy: which scan serves the next step of `remaining` queries, and how many of them it takes.  The ONE place
// that decides; step_queries (how many queries the host entry point stages) and scan_step (what runs) both ask here.
enum class Scan { PQ, SQ, IVF_MULTI, I8, RQ, WIDE, EXACT };
struct Step {
  Scan kind;
  int nq;
  bool i8;  // the int8 family is usable on this index: its copy is kept current even on a step another scan serves
};
static Step choose_step(const knnx_index* ix, int remaining, int k) {
  if (ix->pq.m) return {Scan::PQ, std::min(PQ_PASS, remaining), false};  // IVF-PQ: its own pass, dispatched beside the fp16 scans
  // IVF-SQ8: always its multi-block pass (one block for <= 32 queries; a block needs a workgroup of its own: KNNX_GRID can set few)
  if (ix->sq.on) return {Scan::SQ, std::min(KNN_NQ * std::max(1, std::min(IVFM_BLK, ix->n_cu)), remaining), false};
  if (ivfm_usable(ix, remaining, k)) return {Scan::IVF_MULTI, std::min(IVFM_BLK * KNN_NQ, remaining), false};
  const bool i8 = i8_usable(ix, remaining, k);
  // (two planes: four waves x 32 = 128 queries per int8 pass -- a batch of more goes to the fp16 register-stationary pass, 36 ms for
  // 256 against 2 x 19.6)
  if (i8 && !(ix->i8.planes == 2 && remaining > 128 && rq_usable(ix, remaining, k)))
    return {Scan::I8, std::min(ix->i8.planes == 2 ? 128 : KNN_RQ_MAX, remaining), i8};
  if (rq_usable(ix, remaining, k)) return {Scan::RQ, std::min(rq_queries_per_pass(ix->d), remaining), i8};
  if (wide_usable(ix, remaining, k)) return {Scan::WIDE, std::min(KNN_NQ_MAX, remaining), i8};
  return {Scan::EXACT, std::min(KNN_NQ, remaining), i8};
}

// how many of `remaining` queries the next scan step takes
static int step_queries(const knnx_index* ix, int remaining, int k) { return choose_step(ix, remaining, k).nq; }

// one step of a search over device buffers: runs the scan choose_step picks; returns the number taken.  An allocation that turns
// its family off (ivfm_alloc: ivfm_ok; i8_ensure: i8_ok) and a build of the int8 copy (it decides the planes) make it choose again.
static int scan_step(knnx_index* ix, const float* q_dev, int remaining, int k, float* D_out, int64_t* I_out, hipStream_t st,
                     int* taken) {
  for (;;) {
    const Step s = choose_step(ix, remaining, k);
    if (s.i8 && !ix->i8.valid) {
      const int r = i8_ensure(ix, st);  // (1: built, valid now; 0: given up, i8_ok cleared)
      if (r < 0) return r;
      continue;
    }
    if (s.kind == Scan::IVF_MULTI && ivfm_alloc(ix)) continue;
    *taken = s.nq;
    switch (s.kind) {
      case Scan::PQ: return scan_topk_pq(ix, q_dev, s.nq, k, D_out, I_out, st);
      case Scan::SQ: return scan_topk_sq(ix, q_dev, s.nq, k, D_out, I_out, st);
      case Scan::IVF_MULTI: return scan_topk_ivf_multi(ix, q_dev, s.nq, k, D_out, I_out, st);
      case Scan::I8: return scan_topk_i8(ix, q_dev, s.nq, k, D_out, I_out, st);
      case Scan::RQ: return scan_topk_rq(ix, q_dev, s.nq, k, D_out, I_out, st);
      case Scan::WIDE: return scan_topk_wide(ix, q_dev, s.nq, k, D_out, I_out, st);
      case Scan::EXACT: return scan_topk(ix, q_dev, s.nq, k, D_out, I_out, st);
    }
  }
}

extern "C" int64_t knnx_i8_served(knnx_index* ix) {
  if (!ix) return -1;
  std::lock_guard<std::mutex> lk(ix->mu);
  return (int64_t)ix->i8.served;
}
extern "C" int64_t knnx_i8_rows(knnx_index* ix) {
  if (!ix) return -1;
  std::lock_guard<std::mutex> lk(ix->mu);
  return ix->i8.valid ? ix->i8.nrows : 0;
}
extern "C" int knnx_i8_planes(knnx_index* ix) {
  if (!ix) return -1;
  std::lock_guard<std::mutex> lk(ix->mu);
  return ix->i8.valid ? ix->i8.planes : 0;
}
extern "C" int knnx_i8_dominant(knnx_index* ix, int* cols4) {
  if (!ix) return -1;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->i8.valid) return 0;
  for (int j = 0; j < ix->i8.dom.n && cols4; ++j) {
    int c = j;  // the column at position j
    for (int f = 0; f < ix->i8.dom.nfix; ++f)
      if (ix->i8.dom.pos[f] == j) c = ix->i8.dom.src[f];
    cols4[j] = c;
  }
  return ix->i8.dom.n;
}

extern "C" int knnx_search_device(knnx_index* ix, const float* q_dev, int n, int k, float* D_dev, int64_t* I_dev,
                                  void* stream) {
  if (!ix || !q_dev || !D_dev || !I_dev || n < 0 || k <= 0) return fail(KNNX_E_ARG, "bad search arguments");
  if (k > KNNX_MAX_K_FAST)
    return fail(KNNX_E_UNSUPPORTED, ix->sq.on ? "k > 64 is not supported on an IVF-SQ8 index" : "device-buffer search supports k <= 64");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  hipStream_t st = stream ? (hipStream_t)stream : ix->stream;
  if (scratch_acquire(ix, st)) return KNNX_E_HIP;
  for (int o = 0; o < n;) {
    int nq = 0;
    int r = scan_step(ix, q_dev + (size_t)o * ix->d, n - o, k, D_dev + (size_t)o * k, I_dev + (size_t)o * k, st, &nq);
    if (r) return r;
    o += nq;
  }
  if (scratch_release(ix, st)) return KNNX_E_HIP;
  return KNNX_OK;
}

// k <= 64, host buffers; caller holds ix->mu
int search_fast_locked(knnx_index* ix, const float* q, int n, int k, float* D, int64_t* I) {
  hipStream_t st = ix->stream;
  const size_t QM = KNN_RQ_MAX;  // the widest scan's query count: staging is sized for it
  const size_t qb = QM * ix->d * sizeof(float);
  const size_t db = QM * k * sizeof(float), ib = QM * k * sizeof(int64_t);
  int r = ensure_pin(ix, qb + db + ib + 64);
  if (r) return r;
  char* pin = (char*)ix->pin.p;
  if (scratch_acquire(ix, st)) return KNNX_E_HIP;
  for (int o = 0; o < n;) {
    const int rem = n - o;
    const int nq = step_queries(ix, rem, k);
    memcpy(pin, q + (size_t)o * ix->d, (size_t)nq * ix->d * sizeof(float));
    HIPCHK(hipMemcpyAsync(ix->flat.q_dev, pin, (size_t)nq * ix->d * sizeof(float), hipMemcpyHostToDevice, st));
    int took = 0;
    // the proof-based scans leave their fallback to this function (knnx_index::defer_fb): the gates come back with the results
    ix->defer_fb = true;
    ix->defer_kind = 0;
    r = scan_step(ix, ix->flat.q_dev, nq, k, ix->flat.D_dev, ix->flat.I_dev, st, &took);
    ix->defer_fb = false;
    if (r) return r;
    // (the step may take fewer than were staged: the int8 path can turn itself off -- out of memory -- between the two decisions)
    if (took <= 0 || took > nq) return fail(KNNX_E_STATE, "internal: scan step size mismatch");
    unsigned* gates = reinterpret_cast<unsigned*>(pin + qb + db + ib);
    const int kind = ix->defer_kind, ngroup = kind ? (ix->defer_nq + KNN_NQ - 1) / KNN_NQ : 0;
    if (kind) HIPCHK(hipMemcpyAsync(gates, kind == 1 ? ix->rq.gate : ix->wide.gate, (size_t)ngroup * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pin + qb, ix->flat.D_dev, (size_t)took * k * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pin + qb + db, ix->flat.I_dev, (size_t)took * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    bool again = false;
    for (int g = 0; g < ngroup; ++g) {
      if (!gates[g]) continue;
      // a query of this group is unproven (rare: the bench counts them as fallbacks): its group's exact scan, then the rows again
      const int q0 = g * KNN_NQ, m = std::min(KNN_NQ, ix->defer_nq - q0);
      r = scan_topk(ix, ix->flat.q_dev + (size_t)q0 * ix->d, m, k, ix->wide.Dfb, ix->wide.Ifb, st);
      if (r) return r;
      HIPCHK(launch_select(kind == 1 ? ix->rq.need : ix->wide.need, q0, m, k, ix->wide.Dfb, ix->wide.Ifb, ix->flat.D_dev, ix->flat.I_dev, st));
      again = true;
    }
    if (again) {
      HIPCHK(hipMemcpyAsync(pin + qb, ix->flat.D_dev, (size_t)took * k * sizeof(float), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(pin + qb + db, ix->flat.I_dev, (size_t)took * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    memcpy(D + (size_t)o * k, pin + qb, (size_t)took * k * sizeof(float));
    memcpy(I + (size_t)o * k, pin + qb + db, (size_t)took * k * sizeof(int64_t));
    o += took;
  }
  if (scratch_release(ix, st)) return KNNX_E_HIP;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Request coalescer: single-query calls from many threads -> one scan per batch
// ---------------------------------------------------------------------------------------------
hipError_t knnx_launch_dedup_pairs(const float* rows, const int64_t* ids, int m, int k, int d, float thr, const unsigned char* want_or_null,
                                   int32_t* pairs, int cap, int* npairs, hipStream_t st);  // postfilter.hip

struct CoReq {
  const float* q;     // [d]
  int k;
  float* D;           // [k]
  int64_t* I;         // [k]
  float* R;           // [k, d] or null
  bool dedup;         // also report the request's duplicate links (knnx_search_dedup)
  float thr;
  int32_t* pairs;     // [2 * pairs_cap] (i, j), i < j
  int pairs_cap;
  int* n_pairs;
  int rc = 0;
  std::string err;
  bool done = false;
};

constexpr int CO_PAIR_CAP = 512;  // links kept per request on the device (a request with more falls back to the range scan)

// One batch: `b` holds m <= KNN_RQ_MAX requests with the same k.  Search (one scan), one gather of the m k result rows on the
// device when a request wants them back or wants its dedup links, the link kernel for all of them at once, then every request's
// slice into its own buffers.  Runs under ix->mu; the requests' threads sleep on ix->co.cv meanwhile.
static int co_run_batch_locked(knnx_index* ix, std::vector<CoReq*>& b);
//  The per-index staging vectors co_qbuf / co_Dbuf / co_Ibuf are shared by every caller: with coalescing off
// knnx_search_dedup reaches this function from concurrent request threads, so the index mutex is taken BEFORE they are touched;
// and nothing may leave this function as a C++ exception (a bad_alloc in a resize would otherwise skip the leader's hand-over in
// co_submit and strand every waiter).
static int co_run_batch(knnx_index* ix, std::vector<CoReq*>& b) {
  std::lock_guard<std::mutex> lk(ix->mu);
  try {
    return co_run_batch_locked(ix, b);
  } catch (const std::exception& e) {
    return fail(KNNX_E_NOMEM, std::string("coalesced batch: ") + e.what());
  }
}
static int co_run_batch_locked(knnx_index* ix, std::vector<CoReq*>& b) {
  const int m = (int)b.size(), k = b[0]->k, d = ix->d;
  ix->co.qbuf.resize((size_t)m * d);
  ix->co.Dbuf.resize((size_t)m * k);
  ix->co.Ibuf.resize((size_t)m * k);
  for (int i = 0; i < m; ++i) memcpy(ix->co.qbuf.data() + (size_t)i * d, b[i]->q, (size_t)d * sizeof(float));
  if (set_dev(ix)) return KNNX_E_HIP;
  int r = search_fast_locked(ix, ix->co.qbuf.data(), m, k, ix->co.Dbuf.data(), ix->co.Ibuf.data());
  if (r) return r;
  bool any_r = false, any_dd = false;
  for (CoReq* c : b) { any_r |= c->R != nullptr; any_dd |= c->dedup; }
  if (any_r || any_dd) {
    hipStream_t st = ix->stream;
    const int64_t nrow = (int64_t)m * k;
    int64_t* ids_dev = nullptr;
    float* rows_dev = nullptr;
    int32_t* pairs_dev = nullptr;
    int* np_dev = nullptr;
    unsigned char* want_dev = nullptr;
    if ((r = ensure_scratch(ix, 0, (size_t)nrow * sizeof(int64_t), (void**)&ids_dev))) return r;
    if ((r = ensure_scratch(ix, 1, (size_t)nrow * d * sizeof(float), (void**)&rows_dev))) return r;
    size_t pin_need = (size_t)nrow * sizeof(int64_t);
    if (any_dd) pin_need = std::max(pin_need, (size_t)m * ((size_t)CO_PAIR_CAP * 4 + 8));
    if (any_r) pin_need = std::max(pin_need, std::min((size_t)nrow * d * sizeof(float), (size_t)32 << 20));
    if ((r = ensure_pin(ix, pin_need))) return r;
    memcpy(ix->pin.p, ix->co.Ibuf.data(), (size_t)nrow * sizeof(int64_t));
    HIPCHK(hipMemcpyAsync(ids_dev, ix->pin.p, (size_t)nrow * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // the pinned buffer is reused below
    if (ix->pq.m && (r = pq_decode_rows(ix, ids_dev, nrow, rows_dev, st))) return r;
    if (ix->sq.on && (r = sq_decode_rows(ix, ids_dev, nrow, rows_dev, st))) return r;
    hipError_t e = (ix->pq.m || ix->sq.on) ? hipSuccess
                   : ix->ivf_nlist ? launch_gather_inv(ix->rows, d, ix->id_base, ix->ntotal, ix->ivf.inv, ids_dev, nrow, rows_dev, st)
                                   : launch_gather(ix->rows, ix->ntotal, d, ix->id_base, ids_dev, nrow, rows_dev, st);
    if (e != hipSuccess) return fail(KNNX_E_HIP, std::string("coalesced gather: ") + hipGetErrorString(e));
    if (any_dd) {
      if ((r = ensure_scratch(ix, 6, (size_t)m * CO_PAIR_CAP * sizeof(int32_t), (void**)&pairs_dev))) return r;
      if ((r = ensure_scratch(ix, 7, (size_t)m * sizeof(int), (void**)&np_dev))) return r;
      if ((r = ensure_scratch(ix, 8, (size_t)m, (void**)&want_dev))) return r;
      unsigned char* want = (unsigned char*)ix->pin.p;
      for (int i = 0; i < m; ++i) want[i] = b[i]->dedup ? 1 : 0;
      HIPCHK(hipMemcpyAsync(want_dev, want, (size_t)m, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemsetAsync(np_dev, 0, (size_t)m * sizeof(int), st));
      HIPCHK(hipStreamSynchronize(st));
      // one threshold per batch: requests with another threshold run in their own launch (a service has one: 0.94)
      std::vector<float> thrs;
      for (CoReq* c : b)
        if (c->dedup && std::find(thrs.begin(), thrs.end(), c->thr) == thrs.end()) thrs.push_back(c->thr);
      for (float t : thrs) {
        for (int i = 0; i < m; ++i) want[i] = (b[i]->dedup && b[i]->thr == t) ? 1 : 0;
        if (thrs.size() > 1) {
          HIPCHK(hipMemcpyAsync(want_dev, want, (size_t)m, hipMemcpyHostToDevice, st));
          HIPCHK(hipStreamSynchronize(st));
        }
        e = knnx_launch_dedup_pairs(rows_dev, ids_dev, m, k, d, t, want_dev, pairs_dev, CO_PAIR_CAP, np_dev, st);
        if (e != hipSuccess) return fail(KNNX_E_HIP, std::string("dedup links: ") + hipGetErrorString(e));
      }
      int* np_h = (int*)ix->pin.p;
      int32_t* pairs_h = (int32_t*)((char*)ix->pin.p + (size_t)m * 8);
      HIPCHK(hipMemcpyAsync(np_h, np_dev, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(pairs_h, pairs_dev, (size_t)m * CO_PAIR_CAP * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for (int i = 0; i < m; ++i) {
        CoReq* c = b[i];
        if (!c->dedup) continue;
        const int n = np_h[i];
        *c->n_pairs = n;  // may exceed pairs_cap / CO_PAIR_CAP: the caller sees that and takes the general path
        const int keep = std::min(n, std::min(c->pairs_cap, CO_PAIR_CAP));
        // the device appends in completion order: sort so that the answer does not depend on scheduling
        std::vector<int32_t> ps(pairs_h + (size_t)i * CO_PAIR_CAP, pairs_h + (size_t)i * CO_PAIR_CAP + std::min(n, CO_PAIR_CAP));
        std::sort(ps.begin(), ps.end());
        for (int j = 0; j < keep; ++j) { c->pairs[2 * j] = ps[j] >> 16; c->pairs[2 * j + 1] = ps[j] & 0xffff; }
      }
    }
    if (any_r) {
      const int64_t chunk_rows = std::max<int64_t>(1, (int64_t)(ix->pin.bytes / ((size_t)d * sizeof(float))));
      for (int i = 0; i < m; ++i) {
        if (!b[i]->R) continue;
        for (int64_t o = 0; o < k; o += chunk_rows) {
          const int64_t n = std::min<int64_t>(chunk_rows, k - o);
          HIPCHK(hipMemcpyAsync(ix->pin.p, rows_dev + ((size_t)i * k + o) * d, (size_t)n * d * sizeof(float), hipMemcpyDeviceToHost, st));
          HIPCHK(hipStreamSynchronize(st));
          memcpy(b[i]->R + (size_t)o * d, ix->pin.p, (size_t)n * d * sizeof(float));
        }
      }
    }
  }
  for (int i = 0; i < m; ++i) {
    memcpy(b[i]->D, ix->co.Dbuf.data() + (size_t)i * k, (size_t)k * sizeof(float));
    memcpy(b[i]->I, ix->co.Ibuf.data() + (size_t)i * k, (size_t)k * sizeof(int64_t));
  }
  return KNNX_OK;
}

// Called by every single-query request.  The first thread to find no leader leads: it serves batches (its own request is in
// the first one) until its request is done, then gives the lead away -- a waiting thread picks it up -- so no caller works for
// the others longer than one batch.
static int co_submit(knnx_index* ix, CoReq& me) {
  std::unique_lock<std::mutex> lk(ix->co.mu);
  ix->co.q.push_back(&me);
  for (;;) {
    if (me.done) break;
    if (ix->co.leader) {
      ix->co.cv.wait(lk);
      continue;
    }
    ix->co.leader = true;
    std::vector<CoReq*> batch;
    const int k0 = ix->co.q.front()->k;
    for (auto it = ix->co.q.begin(); it != ix->co.q.end() && (int)batch.size() < KNN_RQ_MAX;) {
      if ((*it)->k == k0) { batch.push_back(*it); it = ix->co.q.erase(it); } else ++it;
    }
    lk.unlock();
    const int r = co_run_batch(ix, batch);
    const std::string msg = r ? std::string(g_err) : std::string();
    lk.lock();
    ix->co.batches++;
    ix->co.queries += (int64_t)batch.size();
    ix->co.largest = std::max<int64_t>(ix->co.largest, (int64_t)batch.size());
    for (CoReq* c : batch) { c->rc = r; c->err = msg; c->done = true; }
    ix->co.leader = false;
    ix->co.cv.notify_all();
  }
  lk.unlock();
  if (me.rc) g_err = me.err;  // the message is thread-local: hand the leader's to this thread
  return me.rc;
}

extern "C" int knnx_set_coalesce(knnx_index* ix, int on) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  std::lock_guard<std::mutex> lk(ix->co.mu);
  ix->co.on = on != 0;
  return KNNX_OK;
}

extern "C" int knnx_coalesce_stats(knnx_index* ix, int64_t* batches, int64_t* queries, int64_t* largest_batch) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  std::lock_guard<std::mutex> lk(ix->co.mu);
  if (batches) *batches = ix->co.batches;
  if (queries) *queries = ix->co.queries;
  if (largest_batch) *largest_batch = ix->co.largest;
  return KNNX_OK;
}

extern "C" int knnx_search_dedup(knnx_index* ix, const float* q, int k, float* D, int64_t* I, float* R_or_null, float dedup_thr,
                                 int32_t* pairs, int pairs_cap, int* n_pairs) {
  if (!ix || !q || !D || !I || k <= 0 || !pairs || pairs_cap < 0 || !n_pairs) return fail(KNNX_E_ARG, "bad search_dedup arguments");
  if (k > KNNX_MAX_K_FAST) return fail(KNNX_E_UNSUPPORTED, "search_dedup serves k <= 64 (larger answers: knnx_search + knnx_range_search_once)");
  CoReq me{q, k, D, I, R_or_null, true, dedup_thr, pairs, pairs_cap, n_pairs};
  *n_pairs = 0;
  if (ix->co.on) return co_submit(ix, me);
  std::vector<CoReq*> one{&me};
  return co_run_batch(ix, one);
}

// every kind of index, any k <= KNNX_MAX_K, host buffers; caller holds ix->mu and has set the device (knnx_search, knnx_search_filtered)
int search_locked(knnx_index* ix, const float* q, int n, int k, float* D, int64_t* I) {
  return (k <= KNNX_MAX_K_FAST) ? search_fast_locked(ix, q, n, k, D, I)
         : ix->pq.m             ? (ix->pq.thr.on ? search_large_k_thr_locked(ix, pq_thr_pass(), q, n, k, D, I)
                                                 : fail(KNNX_E_UNSUPPORTED, "k > 64 is not supported on an IVF-PQ index"))
         : ix->sq.on            ? (ix->sq.thr.on ? search_large_k_thr_locked(ix, sq_thr_pass(), q, n, k, D, I)
                                                 : fail(KNNX_E_UNSUPPORTED, "k > 64 is not supported on an IVF-SQ8 index"))
                                : search_large_k_locked(ix, q, n, k, D, I);
}

extern "C" int knnx_search(knnx_index* ix, const float* q, int n, int k, float* D, int64_t* I, float* R) {
  if (!ix || (n > 0 && (!q || !D || !I)) || n < 0 || k <= 0) return fail(KNNX_E_ARG, "bad search arguments");
  if (k > KNNX_MAX_K) return fail(KNNX_E_UNSUPPORTED, "k > 131072 is not implemented");
  if (ix->pq.m && k > KNNX_MAX_K_FAST) {  // served through the threshold mode of the ADC scan where the index has it switched on
    std::lock_guard<std::mutex> lk(ix->mu);
    if (!ix->pq.thr.on) return fail(KNNX_E_UNSUPPORTED, "k > 64 is not supported on an IVF-PQ index");
  }
  if (ix->sq.on && k > KNNX_MAX_K_FAST) {  // likewise, through the threshold mode of the code scan
    std::lock_guard<std::mutex> lk(ix->mu);
    if (!ix->sq.thr.on) return fail(KNNX_E_UNSUPPORTED, "k > 64 is not supported on an IVF-SQ8 index");
  }
  if (n == 0) return KNNX_OK;
  if (n == 1 && k <= KNNX_MAX_K_FAST && ix->co.on) {  // concurrent single-query callers share one scan
    CoReq me{q, k, D, I, R, false, 0.f, nullptr, 0, nullptr};
    return co_submit(ix, me);
  }
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    if (set_dev(ix)) return KNNX_E_HIP;
    int r = search_locked(ix, q, n, k, D, I);
    if (r) return r;
  }
  if (R) return knnx_reconstruct(ix, I, (int64_t)n * k, R);
  return KNNX_OK;
}

extern "C" int knnx_reconstruct(knnx_index* ix, const int64_t* ids, int64_t n, float* out) {
  if (!ix || (n > 0 && (!ids || !out)) || n < 0) return fail(KNNX_E_ARG, "bad reconstruct arguments");
  if (n == 0) return KNNX_OK;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(32u << 20) / (ix->d * 4)));
  int64_t* ids_dev = nullptr;
  float* out_dev = nullptr;
  int r = ensure_scratch(ix, 0, (size_t)chunk * sizeof(int64_t), (void**)&ids_dev);
  if (r) return r;
  if ((r = ensure_scratch(ix, 1, (size_t)chunk * ix->d * sizeof(float), (void**)&out_dev))) return r;
  // pageable host memory: stage ids and rows through the pinned buffer so that the copies are truly asynchronous DMAs
  if ((r = ensure_pin(ix, (size_t)chunk * (sizeof(int64_t) + (size_t)ix->d * sizeof(float))))) return r;
  int64_t* ids_pin = (int64_t*)ix->pin.p;
  float* out_pin = (float*)((char*)ix->pin.p + (size_t)chunk * sizeof(int64_t));
  hipError_t e = hipSuccess;
  for (int64_t o = 0; o < n && e == hipSuccess; o += chunk) {
    const int64_t m = std::min(chunk, n - o);
    memcpy(ids_pin, ids + o, (size_t)m * sizeof(int64_t));
    e = hipMemcpyAsync(ids_dev, ids_pin, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, ix->stream);
    if (e == hipSuccess && ix->pq.m && (r = pq_decode_rows(ix, ids_dev, m, out_dev, ix->stream))) return r;
    if (e == hipSuccess && ix->sq.on && (r = sq_decode_rows(ix, ids_dev, m, out_dev, ix->stream))) return r;
    if (e == hipSuccess)
      e = (ix->pq.m || ix->sq.on) ? hipSuccess
          : ix->ivf_nlist ? launch_gather_inv(ix->rows, ix->d, ix->id_base, ix->ntotal, ix->ivf.inv, ids_dev, m, out_dev, ix->stream)
                          : launch_gather(ix->rows, ix->ntotal, ix->d, ix->id_base, ids_dev, m, out_dev, ix->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(out_pin, out_dev, (size_t)m * ix->d * sizeof(float), hipMemcpyDeviceToHost, ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e == hipSuccess) memcpy(out + (size_t)o * ix->d, out_pin, (size_t)m * ix->d * sizeof(float));
  }
  if (e != hipSuccess) return fail(KNNX_E_HIP, std::string("reconstruct: ") + hipGetErrorString(e));
  return KNNX_OK;
}

// Benchmark corpora generated straight into caller HBM: dst row i = corpus row row_begin + i * row_stride, fp16 [n, d].
// kind 0: the isotropic corpus of knnx_synth_fill (row_stride must be 1); kind 2: the same with three dominant columns (the
// anisotropy of CLIP embeddings: the int8 first stage takes its 1-plane dominant-column form on it, include/knnx.h); kind 1: the overlapping mixture of n_clusters
// Gaussians of BASELINE config 5 (knn_kernels.hip: knn_synth_mix_kernel; oracle/knn_oracle.py: synth_mixture_rows).
// Synchronous.
extern "C" int knnx_synth_rows_device(int device, void* dst_f16, int64_t row_begin, int64_t row_stride, int64_t n, int d, uint64_t seed,
                                      int kind, int64_t n_clusters, void* stream) {
  if (!dst_f16 || n < 0 || row_begin < 0 || row_stride < 1 || d <= 0 || d % 2 || d > 1024) return fail(KNNX_E_ARG, "bad synth_rows arguments");
  if (n == 0) return KNNX_OK;
  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  if (kind == 0 || kind == 2) {  // 2: the isotropic corpus with three dominant columns (knn_synth_kernel)
    if (row_stride != 1) return fail(KNNX_E_UNSUPPORTED, "the isotropic corpora are generated with row_stride 1 only");
    // the kernel addresses X[row * d]: shift the base so that corpus row row_begin lands on dst row 0
    HIPCHK(launch_synth((_Float16*)dst_f16 - (size_t)row_begin * d, row_begin, n, d, seed, st, kind == 2 ? 1 : 0));
    HIPCHK(hipStreamSynchronize(st));
    return KNNX_OK;
  }
  if (kind != 1 || n_clusters <= 0) return fail(KNNX_E_ARG, "kind must be 0, 2, or 1 (with n_clusters > 0)");
  DevBuf<void> table;
  HIPCHK(table.alloc(synth_mix_table_bytes(d)));
  hipError_t e = launch_synth_mix((_Float16*)dst_f16, row_begin, row_stride, n, d, seed, n_clusters, (short*)table.p, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(KNNX_E_HIP, std::string("synth_rows: ") + hipGetErrorString(e));
  return KNNX_OK;
}

extern "C" int knnx_merge_topk_device(int device, const float* D_parts, const int64_t* I_parts, int P, int n, int k,
                                      float* D_out, int64_t* I_out, void* stream) {
  if (!D_parts || !I_parts || !D_out || !I_out || P <= 0 || n < 0 || k <= 0) return fail(KNNX_E_ARG, "bad merge arguments");
  if (n == 0) return KNNX_OK;
  HIPCHK(hipSetDevice(device));
  if (k > KNNX_MAX_K_FAST) {
    // large k (the front end's num_result_ids = 3000): every shard's list is sorted (score desc, id asc, -1 padding at its tail), so the
    // P-way merge of sorted lists applies -- the kernel the in-process sharded index uses for the same case (knnx_sharded.hip)
    if (P > 64) return fail(KNNX_E_ARG, "merge of k > 64 results takes at most 64 shards");
    HIPCHK(launch_merge_sorted(D_parts, I_parts, P, n, k, D_out, I_out, (hipStream_t)stream));
    return KNNX_OK;
  }
  HIPCHK(launch_merge_i64(D_parts, I_parts, P, n, k, k, D_out, I_out, (hipStream_t)stream));
  return KNNX_OK;
}

extern "C" int knnx_get_stats(knnx_index* ix, int64_t* proof_queries, int64_t* proof_failures) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  unsigned long long h[2] = {0, 0};
  HIPCHK(hipStreamSynchronize(ix->stream));
  HIPCHK(hipMemcpy(h, ix->flat.stats, sizeof(h), hipMemcpyDeviceToHost));
  if (proof_queries) *proof_queries = (int64_t)h[0];
  if (proof_failures) *proof_failures = (int64_t)h[1];
  return KNNX_OK;
}

extern "C" int knnx_profile_enable(knnx_index* ix, int on) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  ix->prof.on = on != 0;
  return KNNX_OK;
}

extern "C" int knnx_profile_get(knnx_index* ix, int64_t* scan_launches, double* scan_ms) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  int64_t n = 0;
  double ms = 0.0;
  for (auto& ev : ix->prof.events) {
    HIPCHK(hipEventSynchronize(ev.second));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, ev.first, ev.second));
    ms += t;
    ++n;
  }
  ix->prof.events.clear();
  if (scan_launches) *scan_launches = n;
  if (scan_ms) *scan_ms = ms;
  return KNNX_OK;
}
