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

static int sq_front(knnx_index* ix, const float* q_dev, int nq, hipStream_t st) {
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
static int sq_pass_top64(knnx_index* ix, int nq, float* D64, hipStream_t st) {
  const int k = KNNX_MAX_K_FAST;
  int r = sq_topk_scan_merge(ix, nq, k, ix->flat.D_dev, ix->flat.I_dev, st);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(D64, ix->flat.D_dev, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// rows in the probed lists of every query of the pass -> total [nq], summed on the device from the blocks' list masks.  Synchronises.
static int sq_pass_probed_rows(knnx_index* ix, int nq, std::vector<int64_t>& total, hipStream_t st) {
  if (!ix->sqs.trows) HIPCHK(ix->sqs.trows.alloc((size_t)IVFM_BLK * KNN_NQ));
  HIPCHK(launch_sq_probed_rows(ix->ivfm.masks, ix->ivf.size, ix->ivf_nlist, nq, ix->sqs.trows, st));
  std::vector<unsigned long long> t((size_t)nq);
  HIPCHK(hipMemcpyAsync(t.data(), ix->sqs.trows, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  total.assign(t.begin(), t.end());
  return 0;
}

// the threshold launch of the pass (ThrPass::launch_threshold)
static int sq_pass_launch_threshold(knnx_index* ix, int nq, unsigned cap, hipStream_t st) {
  SqScanArgs a = sq_scan_args(ix, nq);
  a.rthr = ix->sq.thr.tthr;
  a.rcnt = ix->sq.thr.tcnt;
  a.rcap = cap;
  a.hit_s = ix->range.s;
  a.hit_i = ix->range.i;
  HIPCHK(launch_sq_range_scan(a, st));
  return 0;
}

const ThrPass& sq_thr_pass() {
  static const ThrPass P = {
    "IVF-SQ8",
    [](const knnx_index* ix) { return ix->sq.on; },
    [](knnx_index* ix) -> ThrState& { return ix->sq.thr; },
    sq_pass_max,
    sq_front,
    sq_pass_top64,
    sq_pass_probed_rows,
    sq_pass_launch_threshold,
  };
  return P;
}

extern "C" int knnx_ivfsq_set_threshold_scan(knnx_index* ix, int on) { return thr_set_switch(ix, sq_thr_pass(), on); }
extern "C" int knnx_ivfsq_threshold_scan(const knnx_index* ix) { return thr_switch(ix, sq_thr_pass()); }
extern "C" int knnx_ivfsq_threshold_stats(knnx_index* ix, int64_t* queries, int64_t* launches, int64_t* query_scans, int64_t* hits) {
  return thr_stats(ix, sq_thr_pass(), queries, launches, query_scans, hits);
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
  return ivf_export_codes_locked(ix, ix->sq.codes, ix->d, ix->sq.tile0_h, ix->sq.size_h, "IVF-SQ8", ids, lists, codes);
}

// precomputed codes [n][d] (host) into an index between knnx_ivf_begin and knnx_ivf_end (an index loaded from its saved codes)
extern "C" int knnx_ivfsq_add_codes(knnx_index* ix, const uint8_t* codes, int64_t n, const int64_t* ids, const int32_t* lists,
                                    const int32_t* pos) {
  if (!ix || (n > 0 && (!codes || !ids || !lists || !pos)) || n < 0) return fail(KNNX_E_ARG, "bad ivfsq_add_codes arguments");
  if (n == 0) return KNNX_OK;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (!ix->sq.on || !ix->ivfb.nlist) return fail(KNNX_E_STATE, "set the IVF-SQ8 quantizer and call knnx_ivf_begin first");
  return ivf_import_codes_locked(ix, ix->sq.codes, ix->d, codes, n, ids, lists, pos);
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
