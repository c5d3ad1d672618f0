// knnx_range.hip -- range scans and the large-k search built on them (host side; see knnx_host.h).

#include "knnx_host.h"
#include "knnx_thr_group.h"

static const size_t RANGE_POOL_MAX = (size_t)1 << 29;  // 512 Mi hits = 4 GiB of scratch
constexpr int64_t RANGE_BATCH_MAX_ROWS = 1 << 16;  // range_scan_batched: indexes up to this many rows (a scan is launch-bound there)

// the hit pools with `want` entries each, or none (the int8 copy is reclaimed first when they do not fit)
static int range_pool_alloc(knnx_index* ix, size_t want) {
  ix->range = RangePools();
  hipError_t e = malloc_or_reclaim(ix, ix->range.s, want);
  if (e == hipSuccess) e = malloc_or_reclaim(ix, ix->range.i, want);
  if (e != hipSuccess) ix->range = RangePools();
  HIPCHK(e);
  ix->range.pool = want;
  return 0;
}

// *cap = the entries each of `slices` queries has in the pools (allocated here when there are none yet)
static int range_pool_slice(knnx_index* ix, size_t slices, unsigned* cap) {
  int r;
  if (ix->range.pool == 0 && (r = range_pool_alloc(ix, (size_t)1 << 21))) return r;
  *cap = (unsigned)std::min<size_t>(ix->range.pool / slices, 0xffffffffu);
  return 0;
}

// a scan counted mx hits for one of its `slices` queries and its slice overflowed: grow the pools until mx fit (the caller scans
// again: the counts are exact even when the slices overflowed).  what: "range_search" / "large-k search", for the message
static int range_pool_fit(knnx_index* ix, size_t slices, size_t mx, const char* what) {
  const size_t want = pool_want(ix->range.pool, slices, mx);
  if (want > RANGE_POOL_MAX) return fail(KNNX_E_NOMEM, std::string(what) + " result exceeds the 512 Mi-hit scratch limit");
  return range_pool_alloc(ix, want);
}

// range scan of <= KNN_NQ queries; leaves per-query counts in `counts` and the hits on the device
// (query i's hits at range_s/range_i[i*cap .. i*cap+counts[i]), cap = range_pool / nq)
static int range_scan(knnx_index* ix, const float* q_host, int nq, float thr, std::vector<unsigned>& counts,
                      unsigned* cap_out) {
  hipStream_t st = ix->stream;
  int r = ensure_pin(ix, (size_t)KNN_NQ * ix->d * sizeof(float));
  if (r) return r;
  if (scratch_acquire(ix, st)) return KNNX_E_HIP;
  memcpy(ix->pin.p, q_host, (size_t)nq * ix->d * sizeof(float));
  HIPCHK(hipMemcpyAsync(ix->flat.q_dev, ix->pin.p, (size_t)nq * ix->d * sizeof(float), hipMemcpyHostToDevice, st));
  for (;;) {
    unsigned cap = 0;
    if ((r = range_pool_slice(ix, (size_t)nq, &cap))) return r;
    if (ix->ivf_nlist) {  // IVF: the range is taken over the rows of the nprobe best lists of each query (faiss IndexIVF semantics)
      r = ivf_build_worklist(ix, ix->flat.q_dev, nq, st, nullptr);
      if (r) return r;
    }
    HIPCHK(launch_prep(ix->flat.q_dev, nq, ix->d, ix->flat.qfrag, ix->flat.thr_g, ix->flat.range_cnt, 0, nullptr, st));
    ScanArgs a{};
    a.X = ix->rows;
    a.N = ix->ivf_nlist ? ix->capacity : ix->ntotal;
    a.work = ix->ivf_nlist ? ix->ivf1.work : nullptr;
    a.nwork = ix->ivf1.nwork;
    a.d = ix->d;
    a.qfrag = ix->flat.qfrag;
    a.nq = nq;
    a.k = 1;
    a.cap = 2;
    a.grid = ix->n_cu;
    a.mode = 1;
    a.thr_g = ix->flat.thr_g;
    a.range_thr = thr;
    a.range_cnt = ix->flat.range_cnt;
    a.range_cap = cap;
    a.range_s = ix->range.s;
    a.range_i = ix->range.i;
    HIPCHK(launch_scan(a, st));
    counts.assign(KNN_NQ, 0u);
    HIPCHK(hipMemcpyAsync(counts.data(), ix->flat.range_cnt, KNN_NQ * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    unsigned mx = 0;
    for (int i = 0; i < nq; ++i) mx = std::max(mx, counts[i]);
    if (mx <= cap) {
      *cap_out = cap;
      return 0;
    }
    if ((r = range_pool_fit(ix, (size_t)nq, mx, "range_search"))) return r;
  }
}

// Many queries against a SMALL flat index (the per-request dedup of clip_back.py:290-294: the k result vectors against themselves,
// k up to 3 000): all 32-query groups are launched back to back, every group with its own counters and its own slice of the hit
// pool, and the host synchronises ONCE for the counts -- the one-group-at-a-time loop costs two synchronisations per group
// (94 groups at k = 3 000: 10 ms of a 45 ms request, profiles/r03h_request.log).  counts [n]; *cnt_dev_out = the device counters
// (scratch slot 4) for range_fetch.
static int range_scan_batched(knnx_index* ix, const float* q_host, int n, float thr, std::vector<unsigned>& counts, unsigned* cap_out,
                              unsigned** cnt_dev_out) {
  hipStream_t st = ix->stream;
  const int ngroups = (n + KNN_NQ - 1) / KNN_NQ;
  const size_t nr = (size_t)ngroups * KNN_NQ;
  float* q_all = nullptr;
  unsigned* cnt_all = nullptr;
  int r = ensure_scratch(ix, 3, nr * ix->d * sizeof(float), (void**)&q_all);
  if (!r) r = ensure_scratch(ix, 4, nr * sizeof(unsigned), (void**)&cnt_all);
  if (r) return r;
  if (scratch_acquire(ix, st)) return KNNX_E_HIP;
  HIPCHK(hipMemcpyAsync(q_all, q_host, (size_t)n * ix->d * sizeof(float), hipMemcpyHostToDevice, st));
  for (;;) {
    unsigned cap = 0;
    if ((r = range_pool_slice(ix, nr, &cap))) return r;
    unsigned mx = 0;
    if (cap > 0) {
      for (int g = 0; g < ngroups; ++g) {
        const int q0 = g * KNN_NQ, nq = std::min(KNN_NQ, n - q0);
        HIPCHK(launch_prep(q_all + (size_t)q0 * ix->d, nq, ix->d, ix->flat.qfrag, ix->flat.thr_g, cnt_all + q0, 0, nullptr, st));
        ScanArgs a{};
        a.X = ix->rows;
        a.N = ix->ntotal;
        a.d = ix->d;
        a.qfrag = ix->flat.qfrag;
        a.nq = nq;
        a.k = 1;
        a.cap = 2;
        a.grid = ix->n_cu;
        a.mode = 1;
        a.thr_g = ix->flat.thr_g;
        a.range_thr = thr;
        a.range_cnt = cnt_all + q0;
        a.range_cap = cap;
        a.range_s = ix->range.s + (size_t)q0 * cap;
        a.range_i = ix->range.i + (size_t)q0 * cap;
        HIPCHK(launch_scan(a, st));
      }
      counts.assign(nr, 0u);
      HIPCHK(hipMemcpyAsync(counts.data(), cnt_all, nr * sizeof(unsigned), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for (int i = 0; i < n; ++i) mx = std::max(mx, counts[i]);
      if (mx <= cap) {
        *cap_out = cap;
        *cnt_dev_out = cnt_all;
        return 0;
      }
    } else {
      mx = 1;
    }
    if ((r = range_pool_fit(ix, nr, mx, "range_search"))) return r;
  }
}

// copy the hits of the last range_scan to the host, ids ascending inside each query
static int range_fetch(knnx_index* ix, int nq, const std::vector<unsigned>& counts, unsigned cap, float* D,
                       int64_t* I, const unsigned* cnt_dev = nullptr) {
  if (!cnt_dev) cnt_dev = ix->flat.range_cnt;
  std::vector<int64_t> loc(nq + 1);
  loc[0] = 0;
  for (int i = 0; i < nq; ++i) loc[i + 1] = loc[i] + counts[i];
  if (loc[nq] == 0) return 0;
  int64_t* lims_dev = nullptr;
  float* D_dev = nullptr;
  int64_t* I_dev = nullptr;
  int rr = ensure_scratch(ix, 0, (nq + 1) * sizeof(int64_t), (void**)&lims_dev);
  if (!rr) rr = ensure_scratch(ix, 1, (size_t)loc[nq] * sizeof(float), (void**)&D_dev);
  if (!rr) rr = ensure_scratch(ix, 2, (size_t)loc[nq] * sizeof(int64_t), (void**)&I_dev);
  if (rr) return rr;
  hipError_t e = hipMemcpyAsync(lims_dev, loc.data(), (nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ix->stream);
  if (e == hipSuccess)
    e = launch_range_sort(ix->range.s, ix->range.i, cnt_dev, cap, lims_dev, ix->id_base,
                          ix->ivf_nlist ? ix->ivf.idmap : nullptr, nq, D_dev, I_dev, ix->stream);
  // hit lists too long for rank-by-counting: radix sort by id, one query at a time
  unsigned longest = 0;
  for (int i = 0; i < nq; ++i) longest = std::max(longest, counts[i] > RANGE_SORT_SMALL ? counts[i] : 0u);
  if (e == hipSuccess && longest) {
    DevBuf<uint32_t> k0, k1;
    DevBuf<float> v0, v1;
    DevBuf<unsigned> hist;
    dev_alloc(e, k0, longest);
    dev_alloc(e, k1, longest);
    dev_alloc(e, v0, longest);
    dev_alloc(e, v1, longest);
    dev_alloc(e, hist, (size_t)16 * ((longest + 2047) / 2048));
    int key_bits = 1;
    while (key_bits < 32 && ((int64_t)1 << key_bits) < std::max<int64_t>(ix->ntotal, 2)) ++key_bits;
    for (int i = 0; i < nq && e == hipSuccess; ++i)
      if (counts[i] > RANGE_SORT_SMALL)
        e = launch_range_sort_long(ix->range.s + (size_t)i * cap, ix->range.i + (size_t)i * cap, counts[i], ix->id_base,
                                   ix->ivf_nlist ? ix->ivf.idmap : nullptr, key_bits, k0, k1, v0, v1, hist, D_dev + loc[i],
                                   I_dev + loc[i], ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(D, D_dev, (size_t)loc[nq] * sizeof(float), hipMemcpyDeviceToHost, ix->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(I, I_dev, (size_t)loc[nq] * sizeof(int64_t), hipMemcpyDeviceToHost, ix->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
  if (e != hipSuccess) return fail(KNNX_E_HIP, std::string("range fetch: ") + hipGetErrorString(e));
  return 0;
}

// ---- IVF-PQ / IVF-SQ8 with the threshold-scan switch on: the family's list scan in threshold mode feeds the same pools.  P says what
// the two differ in (knnx_host.h: ThrPass) ----
// stage a group of <= P.pass_max queries and run the front half of their pass
static int thr_pass_begin(knnx_index* ix, const ThrPass& P, const float* q_host, int nq) {
  hipStream_t st = ix->stream;
  int r = ensure_pin(ix, (size_t)P.pass_max(ix) * ix->d * sizeof(float));
  if (r) return r;
  if (scratch_acquire(ix, st)) return KNNX_E_HIP;
  memcpy(ix->pin.p, q_host, (size_t)nq * ix->d * sizeof(float));
  HIPCHK(hipMemcpyAsync(ix->flat.q_dev, ix->pin.p, (size_t)nq * ix->d * sizeof(float), hipMemcpyHostToDevice, st));
  return P.front(ix, ix->flat.q_dev, nq, st);
}

// one threshold scan of the pass: thr_h [nq] (host; +INFINITY: a finished query) -> counts [nq] (exact), hits in ix->range at q * cap;
// the device counters stay in the family's tcnt.  Synchronises.
static int thr_pass_scan(knnx_index* ix, const ThrPass& P, int nq, const float* thr_h, unsigned cap, std::vector<unsigned>& counts) {
  hipStream_t st = ix->stream;
  ThrState& T = P.thr(ix);
  HIPCHK(T.alloc());
  HIPCHK(hipMemcpyAsync(T.tthr, thr_h, (size_t)nq * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(ix->prof.begin(ix->prof.on, st));
  int r = P.launch_threshold(ix, nq, cap, st);
  if (r) return r;
  HIPCHK(ix->prof.end(ix->prof.on, st));
  counts.assign((size_t)nq, 0u);
  HIPCHK(hipMemcpyAsync(counts.data(), T.tcnt, (size_t)nq * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  ++T.scans;
  return 0;
}

// range scan of <= P.pass_max queries of a compressed index: the rows of the probed lists whose score is > thr.  Counts and hits as
// range_scan leaves them, the device counters in the family's tcnt.
static int range_scan_thr(knnx_index* ix, const ThrPass& P, const float* q_host, int nq, float thr, std::vector<unsigned>& counts,
                          unsigned* cap_out) {
  int r = thr_pass_begin(ix, P, q_host, nq);
  if (r) return r;
  const std::vector<float> th((size_t)nq, thr);
  for (;;) {
    unsigned cap = 0;
    if ((r = range_pool_slice(ix, (size_t)nq, &cap))) return r;
    if ((r = thr_pass_scan(ix, P, nq, th.data(), cap, counts))) return r;
    unsigned mx = 0;
    for (int i = 0; i < nq; ++i) mx = std::max(mx, counts[i]);
    if (mx <= cap) {
      *cap_out = cap;
      return 0;
    }
    if ((r = range_pool_fit(ix, (size_t)nq, mx, "range_search"))) return r;  // (the rescan runs over the same front half)
  }
}

// the pass table of a compressed index, null for a flat or IVF-Flat one
static const ThrPass* thr_pass_of(const knnx_index* ix) { return ix->pq.m ? &pq_thr_pass() : ix->sq.on ? &sq_thr_pass() : nullptr; }

// the range scan of one step of knnx_range_search[_once]: <= range_step(ix) queries
static int range_step(const knnx_index* ix, const ThrPass* P) { return P ? P->pass_max(ix) : KNN_NQ; }
static int range_scan_any(knnx_index* ix, const ThrPass* P, const float* q_host, int nq, float thr, std::vector<unsigned>& counts,
                          unsigned* cap_out) {
  return P ? range_scan_thr(ix, *P, q_host, nq, thr, counts, cap_out) : range_scan(ix, q_host, nq, thr, counts, cap_out);
}

// what an IVF-PQ or IVF-SQ8 index answers to a range_search it does not serve (0: it serves it, or is neither).  Caller holds ix->mu.
static int pq_range_refusal(const knnx_index* ix) {
  if (ix->sq.on) return ix->sq.thr.on ? 0 : fail(KNNX_E_UNSUPPORTED, "range_search is not supported on an IVF-SQ8 index");
  if (!ix->pq.m) return 0;
  if (!ix->pq.thr.on) return fail(KNNX_E_UNSUPPORTED, "range_search is not supported on an IVF-PQ index");
  if (ix->pq.refine)
    return fail(KNNX_E_UNSUPPORTED, "range_search is not supported on an IVF-PQ index with a refine store (it would need the exact score of every probed row)");
  return 0;
}

extern "C" int knnx_range_search(knnx_index* ix, const float* q, int n, float thresh, int64_t* lims, float* D,
                                 int64_t* I) {
  if (!ix || !lims || (n > 0 && !q) || n < 0) return fail(KNNX_E_ARG, "bad range_search arguments");
  if ((D == nullptr) != (I == nullptr)) return fail(KNNX_E_ARG, "D and I must both be null or both be set");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (pq_range_refusal(ix)) return KNNX_E_UNSUPPORTED;
  if (set_dev(ix)) return KNNX_E_HIP;
  const bool fill = D != nullptr;
  const ThrPass* P = thr_pass_of(ix);
  const int step = range_step(ix, P);
  int64_t run = 0;
  std::vector<unsigned> counts;
  if (!fill) lims[0] = 0;
  for (int o = 0; o < n; o += step) {
    const int nq = std::min(step, n - o);
    unsigned cap = 0;
    const float* qo = q + (size_t)o * ix->d;
    int r = range_scan_any(ix, P, qo, nq, thresh, counts, &cap);
    if (r) return r;
    if (!fill) {
      for (int i = 0; i < nq; ++i) {
        run += counts[i];
        lims[o + i + 1] = run;
      }
      continue;
    }
    // filling: the caller passes the lims of the counting call; verify them as we go
    for (int i = 0; i < nq; ++i)
      if (lims[o + i + 1] - lims[o + i] != (int64_t)counts[i])
        return fail(KNNX_E_STATE, "lims do not match this query/threshold (index changed between the two calls?)");
    r = range_fetch(ix, nq, counts, cap, D + lims[o], I + lims[o], P ? P->thr(ix).tcnt.p : nullptr);
    if (r) return r;
  }
  return KNNX_OK;
}

// range_search in ONE pass when the caller's buffers are large enough: lims [n + 1] is always filled; D / I (capacity entries)
// receive the hits if lims[n] <= capacity (return KNNX_OK), otherwise nothing is written to them and the return value is 1 --
// the caller then allocates lims[n] entries and uses knnx_range_search's filling call.  Saves the counting scan of the two-call
// protocol for callers with a good guess (the per-request dedup of clip_back.py:290-294: ~k hits for k result vectors).
extern "C" int knnx_range_search_once(knnx_index* ix, const float* q, int n, float thresh, int64_t* lims, float* D, int64_t* I,
                                      int64_t capacity) {
  if (!ix || !lims || (n > 0 && !q) || n < 0 || capacity < 0 || (capacity > 0 && (!D || !I))) return fail(KNNX_E_ARG, "bad range_search_once arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (pq_range_refusal(ix)) return KNNX_E_UNSUPPORTED;
  if (set_dev(ix)) return KNNX_E_HIP;
  const ThrPass* P = thr_pass_of(ix);
  const int step = range_step(ix, P);
  int64_t run = 0;
  bool fits = true;
  std::vector<unsigned> counts;
  lims[0] = 0;
  if (!ix->ivf_nlist && n > KNN_NQ && ix->ntotal <= RANGE_BATCH_MAX_ROWS) {  // small flat index, many queries: one synchronisation
    unsigned cap = 0;
    unsigned* cnt_dev = nullptr;
    int r = range_scan_batched(ix, q, n, thresh, counts, &cap, &cnt_dev);
    if (r) return r;
    for (int i = 0; i < n; ++i) {
      run += counts[i];
      lims[i + 1] = run;
    }
    if (run > capacity) return 1;
    counts.resize(n);
    return range_fetch(ix, n, counts, cap, D, I, cnt_dev);
  }
  for (int o = 0; o < n; o += step) {
    const int nq = std::min(step, n - o);
    unsigned cap = 0;
    const float* qo = q + (size_t)o * ix->d;
    int r = range_scan_any(ix, P, qo, nq, thresh, counts, &cap);
    if (r) return r;
    const int64_t first = run;
    for (int i = 0; i < nq; ++i) {
      run += counts[i];
      lims[o + i + 1] = run;
    }
    if (run > capacity) fits = false;
    if (fits) {
      r = range_fetch(ix, nq, counts, cap, D + first, I + first, P ? P->thr(ix).tcnt.p : nullptr);
      if (r) return r;
    }
  }
  return fits ? KNNX_OK : 1;
}

// k > 64 (the front-end's num_result_ids = 3000, clip_back.py:358 asks for up to 1e5): one range scan with a threshold that
// lets >= k rows through, the hits ranked on the host (k log k, tiny next to a scan).  Exact: every row scoring above the
// threshold is a hit, so cnt >= k hits contain the top k.  The threshold:
//   * flat index with N >= 128 k rows: the j-th best EXACT score of a strided sample (every S-th 32-row tile, the 32-query scan
//     with tstride = S: 1 / S of the bytes), S and j <= 48 chosen so that j S ~ 1.5 k rows are expected above it.  The count
//     above the j-th best of a 1 / S sample is ~ S Gamma(j) whatever the score distribution (the argument of the RQ scan's
//     thresholds, knn_kernels.h), so cnt < k has a probability of a few per cent; then the 64-th sample score is tried
//     (~ S * 64 hits) before the descent below takes over.  Cost: ~1.01 scans instead of the 2 - 6 of round 2 -- and instead of
//     the 10.9 s measured at 100 M rows in round 3 (profiles/r03b_request.log), where a query with one very close neighbour
//     (top - s64 = 0.8) made the first descent step jump below zero and 50 M rows had to be fetched and sorted;
//   * otherwise (small or IVF index): descent from the top-64 scores.  The first step extrapolates the LOCAL score density
//     (32 rows lie between the 32nd and the 64th score), doubling while cnt < k; when a step overshoots by more than 16 x the
//     threshold is bisected back (at most 4 times) before the hits are fetched.
// Caller holds ix->mu.
static int sample_scores_locked(knnx_index* ix, const float* qq, int tstride, float* d64) {
  hipStream_t st = ix->stream;
  int r = ensure_pin(ix, (size_t)ix->d * sizeof(float) + KNNX_MAX_K_FAST * sizeof(float));
  if (r) return r;
  if (scratch_acquire(ix, st)) return KNNX_E_HIP;
  memcpy(ix->pin.p, qq, (size_t)ix->d * sizeof(float));
  HIPCHK(hipMemcpyAsync(ix->flat.q_dev, ix->pin.p, (size_t)ix->d * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(launch_prep(ix->flat.q_dev, 1, ix->d, ix->flat.qfrag, ix->flat.thr_g, nullptr, 0, nullptr, st));
  ScanArgs a{};
  a.X = ix->rows;
  a.N = ix->ntotal;
  a.d = ix->d;
  a.qfrag = ix->flat.qfrag;
  a.nq = 1;
  a.k = KNNX_MAX_K_FAST;
  a.cap = scan_cap(ix->d, KNNX_MAX_K_FAST);
  a.grid = ix->n_cu;
  a.mode = 0;
  a.tstride = tstride;
  a.thr_g = ix->flat.thr_g;
  a.part_s = ix->flat.part_s;
  a.part_i = ix->flat.part_i;
  a.part_n = ix->flat.part_n;
  if (a.cap < 0) return fail(KNNX_E_UNSUPPORTED, "k too large for the LDS queues at this d");
  HIPCHK(launch_scan(a, st));
  HIPCHK(launch_merge_u32(ix->flat.part_s, ix->flat.part_i, ix->flat.part_n, ix->n_cu, KNN_NQ, KNNX_MAX_K_FAST, 1, KNNX_MAX_K_FAST, 0, nullptr, ix->flat.D_dev,
                          ix->flat.I_dev, nullptr, st));
  float* out = (float*)((char*)ix->pin.p + (size_t)ix->d * sizeof(float));
  HIPCHK(hipMemcpyAsync(out, ix->flat.D_dev, KNNX_MAX_K_FAST * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  memcpy(d64, out, KNNX_MAX_K_FAST * sizeof(float));
  if (scratch_release(ix, st)) return KNNX_E_HIP;
  return 0;
}

int search_large_k_locked(knnx_index* ix, const float* q, int n, int k, float* D, int64_t* I) {
  std::vector<float> d64((size_t)KNNX_MAX_K_FAST);
  std::vector<int64_t> i64((size_t)KNNX_MAX_K_FAST);
  const int64_t N = ix->ntotal;
  const int64_t want = std::min<int64_t>(k, N);
  for (int qi = 0; qi < n; ++qi) {
    const float* qq = q + (size_t)qi * ix->d;
    float* Dq = D + (size_t)qi * k;
    int64_t* Iq = I + (size_t)qi * k;
    std::vector<Hit> hits;
    std::vector<unsigned> counts;
    unsigned cap = 0;
    int r;
    bool done = false;
    auto fetch = [&](int64_t cnt) -> int {
      std::vector<float> hd((size_t)cnt);
      std::vector<int64_t> hi((size_t)cnt);
      int rr = range_fetch(ix, 1, counts, cap, hd.data(), hi.data());
      if (rr) return rr;
      hits.reserve((size_t)cnt);
      for (int64_t j = 0; j < cnt; ++j) hits.emplace_back(hd[j], hi[j]);
      return 0;
    };
    float thr_hi = FLT_MAX;  // a threshold known to let fewer than k rows through (descent / bisection bracket)
    if (!ix->ivf_nlist && N >= (int64_t)128 * k) {
      // ---- sampled threshold: S tiles apart, j-th best sample score, j S ~ 1.5 k
      const int S = (int)std::max<int64_t>(2, (3 * (int64_t)k / 2 + 47) / 48);
      const int j = (int)std::min<int64_t>(48, std::max<int64_t>(8, (3 * (int64_t)k / 2 + S - 1) / S));
      r = sample_scores_locked(ix, qq, S, d64.data());
      if (r) return r;
      for (int attempt = 0; attempt < 2 && !done; ++attempt) {
        const float sj = d64[attempt == 0 ? j - 1 : KNNX_MAX_K_FAST - 1];
        if (!(sj > -FLT_MAX)) break;  // fewer sample rows than that
        const float thr = nextafterf(sj, -FLT_MAX);  // the range is strict (>): keep the sample row itself
        r = range_scan(ix, qq, 1, thr, counts, &cap);
        if (r) return r;
        if ((int64_t)counts[0] >= want) {
          if ((r = fetch(counts[0]))) return r;
          done = true;
        } else {
          thr_hi = thr;
        }
      }
    }
    if (!done) {
      r = search_fast_locked(ix, qq, 1, KNNX_MAX_K_FAST, d64.data(), i64.data());
      if (r) return r;
      int have = 0;
      while (have < KNNX_MAX_K_FAST && i64[have] >= 0) ++have;
      if (have < KNNX_MAX_K_FAST) {  // the whole index (or all probed lists) is smaller than 64 rows
        for (int j = 0; j < have; ++j) hits.emplace_back(d64[j], i64[j]);
      } else {
        const float s32 = d64[KNNX_MAX_K_FAST / 2 - 1], s64 = d64[KNNX_MAX_K_FAST - 1];
        // local density: 32 rows within s32 - s64; k - 64 more rows are ~ (k - 64) / 32 such gaps away (fewer: the density grows)
        float step = std::max((s32 - s64) * std::min(64.f, (float)(k - KNNX_MAX_K_FAST) / 32.f) * 0.5f, 1e-4f * std::max(1.f, fabsf(s64)));
        float thr = std::min(s64 - step, thr_hi < FLT_MAX ? nextafterf(thr_hi, -FLT_MAX) : FLT_MAX);
        float lo_ok = -FLT_MAX;  // lowest threshold tried so far (lets >= k rows through once found)
        int64_t prev_cnt = -1;
        int stalled = 0, bisections = 0;
        thr_hi = std::min(thr_hi, s64);
        for (int it = 0;; ++it) {
          r = range_scan(ix, qq, 1, thr, counts, &cap);
          if (r) return r;
          const int64_t cnt = counts[0];
          // an IVF index only reaches the rows of the probed lists: when three ever larger steps add nothing, take what there
          // is.  Flat indexes never take this shortcut: cnt >= min(k, N) is reached after O(log) doublings.
          stalled = (ix->ivf_nlist && cnt == prev_cnt) ? stalled + 1 : 0;
          prev_cnt = cnt;
          if (cnt < want && thr > -FLT_MAX && stalled < 3 && it < 60) {
            thr_hi = thr;
            step *= 2.f;
            thr = (thr - step > -FLT_MAX) ? thr - step : -FLT_MAX;
            continue;
          }
          if (cnt < want && thr > -FLT_MAX) {  // stalled (IVF) or out of patience: everything the scan can reach
            thr = -FLT_MAX;
            stalled = 0;
            continue;
          }
          // enough rows.  Far too many (an overshooting step)?  Bisect back towards the last threshold that had too few.
          if (cnt > 16 * want && cnt > 65536 && bisections < 4 && thr_hi < FLT_MAX && thr > -FLT_MAX) {
            lo_ok = thr;
            thr = 0.5f * (thr + thr_hi);
            ++bisections;
            // (a middle that has too few rows raises thr_hi above and steps down again, towards lo_ok)
            step = 0.5f * (thr - lo_ok);
            continue;
          }
          if ((r = fetch(cnt))) return r;
          break;
        }
      }
    }
    rank_hits(hits, k);  // score descending, ties by ascending id; only the first k are reported
    write_topk(hits, k, Dq, Iq);
  }
  return KNNX_OK;
}

// with a refine store: the kc candidates of every query of the group, re-scored against the ORIGINAL query (still in flat.q_dev, a
// few queries per launch: pq_rescore_kernel), ranked again by (exact score descending, id ascending) and written to rows o .. of D / I
static int pq_refine_group(knnx_index* ix, ThrGroup& g, int o, int k, float* D, int64_t* I) {
  hipStream_t st = ix->stream;
  const int gq = g.gq;
  const int64_t kc = g.kc;
  const int qc = (int)std::max<int64_t>(1, std::min<int64_t>(gq, ((int64_t)1 << 22) / kc));
  int64_t* cand_dev = nullptr;
  float* es_dev = nullptr;
  int r;
  if ((r = ensure_scratch(ix, 3, (size_t)qc * kc * sizeof(int64_t), (void**)&cand_dev))) return r;
  if ((r = ensure_scratch(ix, 4, (size_t)qc * kc * sizeof(float), (void**)&es_dev))) return r;
  std::vector<int64_t> cand;
  std::vector<float> es;
  for (int c0 = 0; c0 < gq; c0 += qc) {
    const int m = std::min(qc, gq - c0);
    cand.assign((size_t)m * kc, -1);
    for (int i = 0; i < m; ++i)
      for (size_t j = 0; j < g.hits[c0 + i].size(); ++j) cand[(size_t)i * kc + j] = g.hits[c0 + i][j].second;
    es.resize((size_t)m * kc);
    HIPCHK(hipMemcpyAsync(cand_dev, cand.data(), cand.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(launch_pq_rescore(ix->rows, ix->d, ix->flat.q_dev + (size_t)c0 * ix->d, m, ix->id_base, ix->ntotal, ix->ivf.inv, cand_dev, (int)kc,
                             es_dev, st));
    HIPCHK(hipMemcpyAsync(es.data(), es_dev, es.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < m; ++i) {
      std::vector<Hit>& h = g.hits[c0 + i];
      for (size_t j = 0; j < h.size(); ++j) h[j].first = es[(size_t)i * kc + j];
      rank_hits(h, k);
      write_topk(h, k, D + (size_t)(o + c0 + i) * k, I + (size_t)(o + c0 + i) * k);
    }
  }
  return 0;
}

// k > 64 on an IVF-PQ or IVF-SQ8 index with the threshold-scan switch on (P: the family's pass table).  A group of queries (up to
// P.pass_max; fewer when group x 16 kc hits would not fit the pools) runs the front half of the pass ONCE; the k = 64 pass over it gives
// every query its 32nd and 64th score; then all queries descend together (knnx_thr_group.h drives knnx_descent.h), one threshold scan
// and one synchronisation per step for the whole group, a finished query riding along with thr = +INFINITY.  A query whose probed
// lists hold <= 2 kc rows takes them all in the first scan.  The hits (score, id) are ranked on the host: (score descending, id
// ascending), the first kc = k kept.  IVF-PQ with a refine store keeps kc = k x k_factor and re-scores them (pq_refine_group).
// Caller holds ix->mu.
int search_large_k_thr_locked(knnx_index* ix, const ThrPass& P, const float* q, int n, int k, float* D, int64_t* I) {
  const bool refine = ix->pq.refine;
  const int64_t kc = refine ? (int64_t)k * ix->pq.k_factor : (int64_t)k;
  if (kc > KNNX_MAX_K)
    return fail(KNNX_E_ARG, "k x k_factor = " + std::to_string(k) + " x " + std::to_string(ix->pq.k_factor) + " exceeds " +
                                std::to_string(KNNX_MAX_K) + " candidates per query");
  hipStream_t st = ix->stream;
  ThrState& T = P.thr(ix);
  const int K64 = KNNX_MAX_K_FAST;
  const int gmax = (int)std::max<size_t>(1, std::min<size_t>((size_t)P.pass_max(ix), RANGE_POOL_MAX / ((size_t)16 * (size_t)kc)));
  std::vector<float> d64, thr, hd;
  std::vector<int64_t> total, hi;
  std::vector<unsigned> counts;
  ThrGroup g;
  for (int o = 0; o < n;) {
    const int gq = std::min(gmax, n - o);
    int r = thr_pass_begin(ix, P, q + (size_t)o * ix->d, gq);
    if (r) return r;
    d64.resize((size_t)gq * K64);
    if ((r = P.top64(ix, gq, d64.data(), st))) return r;
    if ((r = P.probed_rows(ix, gq, total, st))) return r;
    g.start(gq, kc, d64.data(), K64, total.data());
    thr.assign((size_t)gq, 0.f);
    while (g.left > 0) {
      unsigned cap = 0;
      if ((r = range_pool_slice(ix, (size_t)gq, &cap))) return r;
      g.thresholds(thr.data());
      if ((r = thr_pass_scan(ix, P, gq, thr.data(), cap, counts))) return r;
      const ThrGroup::Step s = g.absorb(counts.data(), cap);
      T.query_scans += s.query_scans;
      if (s.nsel > 0) {
        HIPCHK(hipMemcpyAsync(T.tfetch, g.sel.data(), (size_t)gq * sizeof(unsigned), hipMemcpyHostToDevice, st));
        hd.resize((size_t)s.nsel);
        hi.resize((size_t)s.nsel);
        if ((r = range_fetch(ix, gq, g.sel, cap, hd.data(), hi.data(), T.tfetch))) return r;
        T.hits += s.nsel;
      }
      g.take(hd.data(), hi.data());
      // a final threshold whose hits overflowed its slice: regrow, scan it again
      if (s.grow && (r = range_pool_fit(ix, (size_t)gq, s.grow, "large-k search"))) return r;
    }
    T.queries += gq;
    if (refine) {
      if ((r = pq_refine_group(ix, g, o, k, D, I))) return r;
    } else {
      for (int i = 0; i < gq; ++i) write_topk(g.hits[i], k, D + (size_t)(o + i) * k, I + (size_t)(o + i) * k);
    }
    o += gq;
  }
  return KNNX_OK;
}

// ---- the switch and the counters behind knnx_ivf{pq,sq}_set_threshold_scan / _threshold_scan / _threshold_stats ----
int thr_set_switch(knnx_index* ix, const ThrPass& P, int on) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!P.is(ix)) return fail(KNNX_E_STATE, std::string("not an ") + P.family + " index");
  P.thr(ix).on = on != 0;
  return KNNX_OK;
}

int thr_switch(const knnx_index* ix, const ThrPass& P) { return ix && P.is(ix) && P.thr(const_cast<knnx_index*>(ix)).on ? 1 : 0; }

int thr_stats(knnx_index* ix, const ThrPass& P, int64_t* queries, int64_t* launches, int64_t* query_scans, int64_t* hits) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!P.is(ix)) return fail(KNNX_E_STATE, std::string("not an ") + P.family + " index");
  const ThrState& T = P.thr(ix);
  if (queries) *queries = T.queries;
  if (launches) *launches = T.scans;
  if (query_scans) *query_scans = T.query_scans;
  if (hits) *hits = T.hits;
  return KNNX_OK;
}
