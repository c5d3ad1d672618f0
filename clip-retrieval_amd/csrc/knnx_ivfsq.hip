// knnx_ivfsq.hip -- IVF-SQ8 on the host side (include/knnx.h, "IVF-SQ8"): the quantiser, the search pass, the decode behind
// reconstruct / R / dedup, loading and exporting codes, and the column min / max the ranges are trained from.  The build itself is
// knnx_ivf_begin / knnx_ivf_add_assigned[_device] / knnx_ivf_end (knnx_ivf.hip), which encode once a quantiser is set.

#include "knnx_host.h"

#include <math.h>

// ---- one pass of 1 .. 32 IVFM_BLK queries already in HBM ----------------------------------------------------------------------
// The coarse half is scan_topk_ivf_multi's (knnx_ivf.hip: ivfm_coarse_worklists): fragments of q, ONE score dump over the centroids,
// radix select of the nprobe best lists, the per-block work lists.  The list scan then runs over the code arena with the fragments of u = q *
// step (knn_sq_kernels.hip) and the merge is the IVF one.  Every batch size takes this path -- 1 .. 32 queries are one block --
// so a query's ids and scores do not depend on the batch it arrives in.
//
// The pass comes in two halves.  The front half (sq_front) leaves the work lists of the blocks in ix->ivfm and the u fragments, biases
// and inverse scales in ix->sqs; the top-k pass follows it with the list scan and the merge, a threshold pass (the switch
// knnx_ivfsq_set_threshold_scan) with any number of threshold launches over the same work lists.
static int sq_blocks(int nq) { return (nq + KNN_NQ - 1) / KNN_NQ; }
static int sq_grid(const knnx_index* ix, int nblk) { return std::max(1, ix->n_cu / nblk) * nblk; }  // (part_* hold n_cu x 64 lists: grid <= n_cu)

int sq_front(knnx_index* ix, const float* q_dev, int nq, hipStream_t st) {
  const int nblk = sq_blocks(nq);
  if (nq < 1 || nblk > IVFM_BLK || nblk > ix->n_cu) return fail(KNNX_E_STATE, "internal: IVF-SQ8 pass misuse");
  const int grid = sq_grid(ix, nblk);
  hipError_t e = ix->ivfm.alloc(ix->d, (size_t)ix->ivf_nlist, ix->capacity);
  if (e == hipSuccess) e = ix->sqs.alloc(ix->d);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP, std::string("IVF-SQ8 search scratch: ") + hipGetErrorString(e));
  }
  int r = ivfm_coarse_worklists(ix, q_dev, nq, nblk, grid, nullptr, st);
  if (r) return r;
  HIPCHK(launch_sq_prep(q_dev, nq, ix->d, ix->sq.vmin, ix->sq.step, ix->sqs.u, ix->sqs.bq, ix->sqs.inv, st));
  HIPCHK(launch_prep_blocks(ix->sqs.u, nq, ix->d, ix->sqs.qfrag, ix->ivfm.thr_f, nullptr, st));  // (resets the list scan's thresholds)
  return 0;
}

// what both modes of the list scan read of the pass whose front half is in ix->ivfm / ix->sqs
static SqScanArgs sq_scan_args(const knnx_index* ix, int nq) {
  SqScanArgs a{};
  a.codes = ix->sq.codes;
  a.d = ix->d;
  a.qfrag = ix->sqs.qfrag;
  a.bq = ix->sqs.bq;
  a.inv = ix->sqs.inv;
  a.nq = nq;
  a.nblk = sq_blocks(nq);
  a.grid = sq_grid(ix, a.nblk);
  a.work = ix->ivfm.work;
  a.nwork = ix->ivfm.nwork;
  a.work_stride = ix->ivfm.stride;
  return a;
}

// the top-k list scan over the work lists of the front half, and the merge of its partial lists
static int sq_topk_scan_merge(knnx_index* ix, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st) {
  const int cap = scan_cap(ix->d, k);
  if (cap < 0) return fail(KNNX_E_STATE, "internal: IVF-SQ8 pass misuse");
  SqScanArgs a = sq_scan_args(ix, nq);
  const int nblk = a.nblk, grid = a.grid;
  a.k = k;
  a.cap = cap;
  a.thr_g = ix->ivfm.thr_f;
  a.part_s = ix->flat.part_s;
  a.part_i = ix->flat.part_i;
  a.part_n = ix->flat.part_n;
  HIPCHK(ix->prof.begin(ix->prof.on, st));
  HIPCHK(launch_sq_scan(a, st));
  HIPCHK(ix->prof.end(ix->prof.on, st));
  HIPCHK(launch_merge_u32(ix->flat.part_s, ix->flat.part_i, ix->flat.part_n, grid - nblk + 1, KNN_NQ, k, nq, k, ix->id_base, ix->ivf.idmap,
                          D_out, I_out, nullptr, st, KNN_NQ, ix->ivfm.nwork, nblk, grid));
  ix->ivfm_last_blk = nblk;
  ix->ivfm_union_valid = ix->prof.on;
  return 0;
}

int scan_topk_sq(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st) {
  if (scan_cap(ix->d, k) < 0) return fail(KNNX_E_STATE, "internal: IVF-SQ8 pass misuse");
  int r = sq_front(ix, q_dev, nq, st);
  if (r) return r;
  return sq_topk_scan_merge(ix, nq, k, D_out, I_out, st);
}

// ---- threshold passes (the switch knnx_ivfsq_set_threshold_scan; knnx_range.hip drives them) ---------------------------------------
// the top-64 scores of the pass whose front half is in place -> D64 host [nq][64], -FLT_MAX padded.  Synchronises.
int sq_pass_top64(knnx_index* ix, int nq, float* D64, hipStream_t st) {
  const int k = KNNX_MAX_K_FAST;
  int r = sq_topk_scan_merge(ix, nq, k, ix->flat.D_dev, ix->flat.I_dev, st);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(D64, ix->flat.D_dev, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// rows in the probed lists of every query of the pass -> total [nq], summed on the device from the blocks' list masks.  Synchronises.
int sq_pass_probed_rows(knnx_index* ix, int nq, std::vector<int64_t>& total, hipStream_t st) {
  HIPCHK(ix->sqs.alloc_threshold());
  HIPCHK(launch_sq_probed_rows(ix->ivfm.masks, ix->ivf.size, ix->ivf_nlist, nq, ix->sqs.trows, st));
  std::vector<unsigned long long> t((size_t)nq);
  HIPCHK(hipMemcpyAsync(t.data(), ix->sqs.trows, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  total.assign(t.begin(), t.end());
  return 0;
}

// one threshold launch of the pass: thr_h [nq] (host; +INFINITY: a finished query) -> counts [nq] (exact), hits in ix->range at q * cap;
// the device counters stay in ix->sqs.tcnt.  Synchronises.
int sq_pass_threshold_scan(knnx_index* ix, int nq, const float* thr_h, unsigned cap, std::vector<unsigned>& counts, hipStream_t st) {
  SqScratch& S = ix->sqs;
  HIPCHK(S.alloc_threshold());
  HIPCHK(hipMemcpyAsync(S.tthr, thr_h, (size_t)nq * sizeof(float), hipMemcpyHostToDevice, st));
  SqScanArgs a = sq_scan_args(ix, nq);
  a.rthr = S.tthr;
  a.rcnt = S.tcnt;
  a.rcap = cap;
  a.hit_s = ix->range.s;
  a.hit_i = ix->range.i;
  HIPCHK(ix->prof.begin(ix->prof.on, st));
  HIPCHK(launch_sq_range_scan(a, st));
  HIPCHK(ix->prof.end(ix->prof.on, st));
  counts.assign((size_t)nq, 0u);
  HIPCHK(hipMemcpyAsync(counts.data(), S.tcnt, (size_t)nq * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  ++ix->sq.thr_scans;
  return 0;
}

extern "C" int knnx_ivfsq_set_threshold_scan(knnx_index* ix, int on) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->sq.on) return fail(KNNX_E_STATE, "not an IVF-SQ8 index");
  ix->sq.threshold_scan = on != 0;
  return KNNX_OK;
}
extern "C" int knnx_ivfsq_threshold_scan(const knnx_index* ix) { return ix && ix->sq.on && ix->sq.threshold_scan ? 1 : 0; }

// counters of the threshold passes since the index was created: queries served with k > 64, threshold launches (one serves a whole
// group), launches summed over the queries that took part in them, hits fetched to the host
extern "C" int knnx_ivfsq_threshold_stats(knnx_index* ix, int64_t* queries, int64_t* launches, int64_t* query_scans, int64_t* hits) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->sq.on) return fail(KNNX_E_STATE, "not an IVF-SQ8 index");
  if (queries) *queries = ix->sq.thr_queries;
  if (launches) *launches = ix->sq.thr_scans;
  if (query_scans) *query_scans = ix->sq.thr_query_scans;
  if (hits) *hits = ix->sq.thr_hits;
  return KNNX_OK;
}

int sq_decode_rows(knnx_index* ix, const int64_t* ids_dev, int64_t n, float* out_dev, hipStream_t st) {
  HIPCHK(launch_sq_decode(ix->sq.codes, ix->d, ix->sq.vmin, ix->sq.step, ix->id_base, ix->ntotal, ix->ivf.inv, ids_dev, n, out_dev, st));
  return KNNX_OK;
}

// ---- the quantiser -------------------------------------------------------------------------------------------------------------
extern "C" int knnx_ivfsq_set_quantizer(knnx_index* ix, const float* vmin, const float* vdiff) {
  if (!ix || !vmin || !vdiff) return fail(KNNX_E_ARG, "bad ivfsq_set_quantizer arguments");
  const int d = ix->d;
  for (int j = 0; j < d; ++j)
    if (!isfinite(vmin[j]) || !isfinite(vdiff[j]) || vdiff[j] < 0.f)
      return fail(KNNX_E_ARG, "IVF-SQ8 needs finite vmin and finite vdiff >= 0 (column " + std::to_string(j) + ")");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (ix->pq.m) return fail(KNNX_E_STATE, "the IVF-SQ8 quantizer cannot be set on an IVF-PQ index");
  if (ix->rows.borrowed || ix->rows || ix->ntotal != 0 || ix->ivf_nlist || ix->ivfb.nlist || ix->sq.on)
    return fail(KNNX_E_STATE, "the IVF-SQ8 quantizer is set once, on an empty index, before knnx_ivf_begin");
  // scale and step in fp32 with IEEE division, here on the host: what numpy float32 computes, bit for bit
  std::vector<float> scale((size_t)d), step((size_t)d);
  for (int j = 0; j < d; ++j) {
    const float vd = vdiff[j];
    scale[j] = vd == 0.f ? 0.f : 255.f / vd;
    step[j] = vd / 255.f;
  }
  hipError_t e = hipSuccess;
  dev_alloc(e, ix->sq.vmin, (size_t)d);
  dev_alloc(e, ix->sq.scale, (size_t)d);
  dev_alloc(e, ix->sq.step, (size_t)d);
  if (e == hipSuccess) e = hipMemcpy(ix->sq.vmin, vmin, (size_t)d * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ix->sq.scale, scale.data(), (size_t)d * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ix->sq.step, step.data(), (size_t)d * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ix->sq = SqData();
    return fail(e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP, std::string("ivfsq_set_quantizer: ") + hipGetErrorString(e));
  }
  ix->sq.vmin_h.assign(vmin, vmin + d);
  ix->sq.vdiff_h.assign(vdiff, vdiff + d);
  ix->sq.on = true;
  return KNNX_OK;
}

extern "C" int knnx_ivfsq_get_quantizer(knnx_index* ix, float* vmin, float* vdiff) {
  if (!ix || !vmin || !vdiff) return fail(KNNX_E_ARG, "bad ivfsq_get_quantizer arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->sq.on) return fail(KNNX_E_STATE, "not an IVF-SQ8 index");
  memcpy(vmin, ix->sq.vmin_h.data(), (size_t)ix->d * sizeof(float));
  memcpy(vdiff, ix->sq.vdiff_h.data(), (size_t)ix->d * sizeof(float));
  return KNNX_OK;
}

extern "C" int knnx_ivfsq(const knnx_index* ix) { return ix && ix->sq.on ? 1 : 0; }

// ---- codes in and out ----------------------------------------------------------------------------------------------------------
// every row of a built index in arena order: ids [ntotal], lists [ntotal], codes [ntotal][d]
extern "C" int knnx_ivfsq_get_codes(knnx_index* ix, int64_t* ids, int32_t* lists, uint8_t* codes) {
  if (!ix || !ids || !lists || !codes) return fail(KNNX_E_ARG, "bad ivfsq_get_codes arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->sq.on || !ix->ivf_nlist) return fail(KNNX_E_STATE, "not a built IVF-SQ8 index (knnx_ivf_end first)");
  if (set_dev(ix)) return KNNX_E_HIP;
  HIPCHK(hipStreamSynchronize(ix->stream));
  const size_t d = (size_t)ix->d;
  std::vector<int64_t> idmap((size_t)ix->capacity);
  HIPCHK(hipMemcpy(idmap.data(), ix->ivf.idmap, idmap.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  int64_t o = 0;
  for (int l = 0; l < ix->ivf_nlist; ++l) {  // a list's rows are contiguous in the arena: one copy per list, straight into place
    const size_t r0 = (size_t)ix->sq.tile0_h[l] * 32, n = ix->sq.size_h[l];
    if (n) HIPCHK(hipMemcpy(codes + (size_t)o * d, ix->sq.codes + r0 * d, n * d, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i, ++o) {
      ids[o] = idmap[r0 + i];
      lists[o] = l;
    }
  }
  return o == ix->ntotal ? KNNX_OK : fail(KNNX_E_STATE, "internal: IVF-SQ8 layout does not add up to ntotal");
}

// precomputed codes [n][d] (host) into an index between knnx_ivf_begin and knnx_ivf_end: the (list, position) rules of
// knnx_ivf_add_assigned, the scatter alone (an index loaded from its saved codes)
extern "C" int knnx_ivfsq_add_codes(knnx_index* ix, const uint8_t* codes, int64_t n, const int64_t* ids, const int32_t* lists,
                                    const int32_t* pos) {
  if (!ix || (n > 0 && (!codes || !ids || !lists || !pos)) || n < 0) return fail(KNNX_E_ARG, "bad ivfsq_add_codes arguments");
  if (n == 0) return KNNX_OK;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (!ix->sq.on || !ix->ivfb.nlist) return fail(KNNX_E_STATE, "set the IVF-SQ8 quantizer and call knnx_ivf_begin first");
  if (ix->ivfb.added + n > ix->ivfb.total) return fail(KNNX_E_ARG, "more rows than the list sizes announced");
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < ix->id_base || ids[i] - ix->id_base >= ix->ivfb.total) return fail(KNNX_E_ARG, "ids must lie in [id_base, id_base + total rows)");
  if (!ivfb_claim_all(ix, lists, pos, n)) return KNNX_E_ARG;
  const int d = ix->d;
  // (ivfb.rows holds IVFB_CHUNK x d x 2 bytes: room for IVFB_CHUNK rows of d code bytes)
  for (int64_t o = 0; o < n; o += IVFB_CHUNK) {
    const int64_t m = std::min(IVFB_CHUNK, n - o);
    HIPCHK(hipMemcpy(ix->ivfb.rows, codes + (size_t)o * d, (size_t)m * d, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->ivfb.ids, ids + o, (size_t)m * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->ivfb.lists, lists + o, (size_t)m * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->ivfb.pos, pos + o, (size_t)m * 4, hipMemcpyHostToDevice));
    HIPCHK(launch_pq_scatter_codes((const uint8_t*)ix->ivfb.rows.p, m, d, ix->ivfb.lists, ix->ivfb.pos, ix->ivfb.ids, ix->ivf.tile0,
                                   ix->id_base, ix->ivfb.total, ix->sq.codes, ix->ivf.idmap, ix->ivf.inv, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
  }
  ix->ivfb.added += n;
  return KNNX_OK;
}

// ---- training: per-column min and max of fp16 rows in HBM (faiss RS_minmax with argument 0) ---------------------------------------
extern "C" int knnx_colminmax_device(int device, const void* rows_dev_f16, int64_t n, int d, float* vmin_out, float* vmax_out,
                                     void* stream) {
  if (!rows_dev_f16 || n <= 0 || d <= 0 || d > 1024 || !vmin_out || !vmax_out) return fail(KNNX_E_ARG, "bad colminmax arguments (n > 0, 0 < d <= 1024)");
  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  DevBuf<int> enc;
  DevBuf<float> out;
  HIPCHK(enc.alloc((size_t)2 * d));
  HIPCHK(out.alloc((size_t)2 * d));
  HIPCHK(launch_sq_colminmax((const _Float16*)rows_dev_f16, n, d, enc, out, out + d, st));
  HIPCHK(hipMemcpyAsync(vmin_out, out, (size_t)d * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(vmax_out, out + d, (size_t)d * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return KNNX_OK;
}
