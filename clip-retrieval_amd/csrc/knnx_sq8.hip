// knnx_sq8.hip -- the flat SQ8 index on the host side (include/knnx.h, "Flat SQ8"): faiss IndexScalarQuantizer(d, QT_8bit,
// METRIC_INNER_PRODUCT), the "SQ8" factory string.  One code byte per dimension in an arena in id order, nothing else per row: the
// quantiser, the arena and its growth, add (encode a staged chunk, keep no fp16 row), the two search steps, the decode behind
// reconstruct / R, codes in and out.  The kernels are those of IVF-SQ8 (knn_sq_kernels.hip) plus the one-pass batch scan.

#include "knnx_host.h"

#include <math.h>

int sq8_refuse(const knnx_index* ix, const std::string& who) {
  if (!ix || !ix->fsq.on) return 0;
  return fail(KNNX_E_UNSUPPORTED, who + " is not supported on a flat SQ8 index");
}

// ---- the arena: [capacity][d] bytes, capacity a multiple of 32, rows past ntotal zero ---------------------------------------------
static int sq8_grow(knnx_index* ix, int64_t need_rows) {
  need_rows = (need_rows + 31) & ~(int64_t)31;
  if (need_rows <= ix->capacity) return 0;
  if (need_rows > (int64_t)0xffffffffll) return fail(KNNX_E_UNSUPPORTED, "more than 2^32 rows per device");
  DevBuf<uint8_t> nc;
  DevBuf<uint4> nw;
  HIPCHK(nc.alloc((size_t)need_rows * ix->d));
  HIPCHK(nw.alloc((size_t)need_rows / 32));
  HIPCHK(hipMemsetAsync(nc, 0, (size_t)need_rows * ix->d, ix->stream));
  if (ix->fsq.codes && ix->ntotal > 0)
    HIPCHK(hipMemcpyAsync(nc, ix->fsq.codes, (size_t)ix->ntotal * ix->d, hipMemcpyDeviceToDevice, ix->stream));
  HIPCHK(hipStreamSynchronize(ix->stream));
  ix->fsq.codes = std::move(nc);
  ix->fsq.work = std::move(nw);
  ix->fsq.work_rows = -1;
  ix->capacity = need_rows;
  return 0;
}

int sq8_reserve_locked(knnx_index* ix, int64_t n_rows) { return sq8_grow(ix, n_rows); }

static int sq8_grow_for(knnx_index* ix, int64_t n) {
  if (ix->ntotal + n <= ix->capacity) return 0;
  return sq8_grow(ix, std::max<int64_t>(ix->ntotal + n, ix->capacity + ix->capacity / 2));
}

// n fp16 rows in HBM -> codes of rows [ntotal, ntotal + n) (the arena is large enough)
static hipError_t sq8_encode_chunk(knnx_index* ix, const _Float16* rows_dev, int64_t at, int64_t n) {
  return launch_sq_encode(rows_dev, n, ix->d, nullptr, nullptr, nullptr, 0, nullptr, 0, 0, ix->fsq.vmin, ix->fsq.scale,
                          ix->fsq.codes + (size_t)at * ix->d, nullptr, nullptr, ix->stream);
}

// knnx_add_f16 / knnx_add_f32 on a flat SQ8 index: chunks staged through pinned memory, rounded to fp16 as the flat index rounds
// them, encoded, not kept
int sq8_add_locked(knnx_index* ix, const void* rows, int64_t n, bool is_f32) {
  int r = sq8_grow_for(ix, n);
  if (r) return r;
  const size_t esz = is_f32 ? 4 : 2;
  const int64_t chunk_rows = std::max<int64_t>(1, (int64_t)(64u << 20) / (int64_t)(ix->d * esz));
  const int64_t cr = std::min(chunk_rows, n);
  if ((r = ensure_pin(ix, (size_t)cr * ix->d * esz))) return r;
  DevBuf<float> tmp32;
  DevBuf<_Float16> tmp16;
  if (is_f32) HIPCHK(tmp32.alloc((size_t)cr * ix->d));
  HIPCHK(tmp16.alloc((size_t)cr * ix->d));
  for (int64_t o = 0; o < n; o += cr) {
    const int64_t m = std::min(cr, n - o);
    const size_t bytes = (size_t)m * ix->d * esz;
    memcpy(ix->pin.p, (const char*)rows + (size_t)o * ix->d * esz, bytes);
    hipError_t e;
    if (is_f32) {
      e = hipMemcpyAsync(tmp32, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->stream);
      if (e == hipSuccess) e = launch_f32_to_f16(tmp32, tmp16, m * ix->d, ix->stream);
    } else {
      e = hipMemcpyAsync(tmp16, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->stream);
    }
    if (e == hipSuccess) e = sq8_encode_chunk(ix, tmp16, ix->ntotal + o, m);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess) return fail(KNNX_E_HIP, std::string("flat SQ8 add: ") + hipGetErrorString(e));
  }
  ix->ntotal += n;
  return KNNX_OK;
}

extern "C" int knnx_sq8_add_device_f16(knnx_index* ix, const void* rows_dev_f16, int64_t n) {
  if (!ix || (!rows_dev_f16 && n > 0) || n < 0) return fail(KNNX_E_ARG, "bad sq8_add_device_f16 arguments");
  if (n == 0) return KNNX_OK;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->fsq.on) return fail(KNNX_E_STATE, "not a flat SQ8 index (knnx_sq8_set_quantizer first)");
  if (set_dev(ix)) return KNNX_E_HIP;
  int r = sq8_grow_for(ix, n);
  if (r) return r;
  HIPCHK(sq8_encode_chunk(ix, (const _Float16*)rows_dev_f16, ix->ntotal, n));
  HIPCHK(hipStreamSynchronize(ix->stream));
  ix->ntotal += n;
  return KNNX_OK;
}

// ---- search ----------------------------------------------------------------------------------------------------------------------
static bool sq8_batch_usable(const knnx_index* ix, int remaining) {
  return ix->rq_ok && remaining > KNN_NQ && ix->ntotal >= ix->rq_min_rows && sq_rq_queries_per_pass(ix->d) > 0;
}
int sq8_step_queries(const knnx_index* ix, int remaining) {
  return std::min(remaining, sq8_batch_usable(ix, remaining) ? sq_rq_queries_per_pass(ix->d) : KNN_NQ);
}

// A step comes in two halves, like an IVF-SQ8 pass.  The front half (sq8_front) leaves u, its fragments, the biases and inverse scales
// of the step's queries in ix->fsq and, for a step of <= 32 queries, the flat work list; the top-k step follows it with the scan of its
// route and the merge, a threshold pass (the switch knnx_sq8_set_threshold_scan) with any number of threshold launches of that route.
static int sq8_front(knnx_index* ix, const float* q_dev, int nq, hipStream_t st) {
  Sq8Flat& f = ix->fsq;
  const int d = ix->d;
  if (nq < 1 || nq > (nq > KNN_NQ ? sq_rq_queries_per_pass(d) : KNN_NQ)) return fail(KNNX_E_STATE, "internal: flat SQ8 step misuse");
  hipError_t e = f.alloc_scratch(d, (size_t)ix->n_cu);
  if (e == hipSuccess && !f.nwork) e = f.nwork.alloc(1);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP, std::string("flat SQ8 search scratch: ") + hipGetErrorString(e));
  }
  HIPCHK(launch_sq_prep(q_dev, nq, d, f.vmin, f.step, f.u, f.bq, f.inv, st));
  HIPCHK(launch_prep_blocks(f.u, nq, d, f.qfrag, f.thr, nullptr, st));  // (resets the thresholds of the blocks it prepares)
  // <= 32 queries: the list scan of IVF-SQ8 walks the arena as one run of tiles
  if (nq <= KNN_NQ && ix->ntotal > 0 && f.work_rows != ix->ntotal) {
    HIPCHK(launch_sq_flat_worklist(ix->ntotal, f.work, f.nwork, st));
    f.work_rows = ix->ntotal;
  }
  return 0;
}

// workgroups of the one-pass batch scan
static int sq8_rq_grid(const knnx_index* ix) { return (int)std::min<int64_t>(ix->n_cu, (ix->ntotal + 31) / 32); }

// what both modes of the list scan read of the step whose front half is in ix->fsq (nq <= 32)
static SqScanArgs sq8_list_args(const knnx_index* ix, int nq) {
  const Sq8Flat& f = ix->fsq;
  SqScanArgs a{};
  a.codes = f.codes;
  a.d = ix->d;
  a.qfrag = f.qfrag;
  a.bq = f.bq;
  a.inv = f.inv;
  a.nq = nq;
  a.grid = ix->n_cu;
  a.work = f.work;
  a.nwork = f.nwork;
  a.nblk = 1;
  a.work_stride = (unsigned)(ix->capacity / 32);
  return a;
}

// the top-k scan of the step's route over what the front half left, and the merge of its partial lists
static int sq8_topk_scan_merge(knnx_index* ix, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st) {
  Sq8Flat& f = ix->fsq;
  const int d = ix->d;
  const int cap = scan_cap(d, k);
  if (k > KNNX_MAX_K_FAST || cap < 0) return fail(KNNX_E_STATE, "internal: flat SQ8 step misuse");
  if (ix->ntotal == 0) {  // nothing to scan: every partial list empty
    HIPCHK(hipMemsetAsync(f.part_n, 0, (size_t)KNN_NQ * sizeof(int), st));
    HIPCHK(launch_merge_u32(f.part_s, f.part_i, f.part_n, 1, KNN_NQ, k, nq, k, ix->id_base, nullptr, D_out, I_out, nullptr, st));
    return 0;
  }
  if (nq > KNN_NQ) {
    // the one-pass batch scan: every code byte once for the whole step
    const int nqp = sq_rq_queries_per_pass(d);
    const int grid = sq8_rq_grid(ix);
    HIPCHK(ix->prof.begin(ix->prof.on, st));
    HIPCHK(launch_sq_rq_scan(f.codes, ix->ntotal, d, f.qfrag, f.bq, f.inv, nq, k, f.thr, f.part_s, f.part_i, f.part_n, grid, st));
    HIPCHK(ix->prof.end(ix->prof.on, st));
    HIPCHK(launch_merge_u32(f.part_s, f.part_i, f.part_n, grid, nqp, k, nq, k, ix->id_base, nullptr, D_out, I_out, nullptr, st));
    return 0;
  }
  SqScanArgs a = sq8_list_args(ix, nq);
  a.k = k;
  a.cap = cap;
  a.thr_g = f.thr;
  a.part_s = ix->flat.part_s;
  a.part_i = ix->flat.part_i;
  a.part_n = ix->flat.part_n;
  HIPCHK(ix->prof.begin(ix->prof.on, st));
  HIPCHK(launch_sq_scan(a, st));
  HIPCHK(ix->prof.end(ix->prof.on, st));
  HIPCHK(launch_merge_u32(ix->flat.part_s, ix->flat.part_i, ix->flat.part_n, ix->n_cu, KNN_NQ, k, nq, k, ix->id_base, nullptr, D_out, I_out,
                          nullptr, st));
  return 0;
}

int scan_topk_sq8(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st) {
  if (k > KNNX_MAX_K_FAST || scan_cap(ix->d, k) < 0) return fail(KNNX_E_STATE, "internal: flat SQ8 step misuse");
  int r = sq8_front(ix, q_dev, nq, st);
  if (r) return r;
  return sq8_topk_scan_merge(ix, nq, k, D_out, I_out, st);
}

// ---- threshold passes (the switch knnx_sq8_set_threshold_scan; knnx_range.hip drives them) ------------------------------------------
// A group takes the route a step of its size takes at k <= 64 (sq8_step_queries): <= 32 queries the list scan over the flat work list,
// more the one-pass batch scan -- so pass_max is the batch scan's queries per pass where that route is usable, 32 otherwise.
static int sq8_pass_max(const knnx_index* ix) { return sq8_step_queries(ix, std::max(sq_rq_queries_per_pass(ix->d), KNN_NQ)); }

// the top-64 scores of the pass whose front half is in place -> D64 host [nq][64], -FLT_MAX padded.  Synchronises.
static int sq8_pass_top64(knnx_index* ix, int nq, float* D64, hipStream_t st) {
  const int k = KNNX_MAX_K_FAST;
  int r = sq8_topk_scan_merge(ix, nq, k, ix->flat.D_dev, ix->flat.I_dev, st);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(D64, ix->flat.D_dev, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// no lists: every query reaches every row
static int sq8_pass_probed_rows(knnx_index* ix, int nq, std::vector<int64_t>& total, hipStream_t) {
  total.assign((size_t)nq, ix->ntotal);
  return 0;
}

// the threshold launch of the pass (ThrPass::launch_threshold); an empty index has no hits
static int sq8_pass_launch_threshold(knnx_index* ix, int nq, unsigned cap, hipStream_t st) {
  Sq8Flat& f = ix->fsq;
  if (ix->ntotal == 0) {
    HIPCHK(hipMemsetAsync(f.thr_scan.tcnt, 0, (size_t)nq * sizeof(unsigned), st));
    return 0;
  }
  if (nq > KNN_NQ) {
    HIPCHK(launch_sq_rq_range_scan(f.codes, ix->ntotal, ix->d, f.qfrag, f.bq, f.inv, nq, f.thr_scan.tthr, f.thr_scan.tcnt, cap, ix->range.s,
                                   ix->range.i, sq8_rq_grid(ix), st));
    return 0;
  }
  SqScanArgs a = sq8_list_args(ix, nq);
  a.rthr = f.thr_scan.tthr;
  a.rcnt = f.thr_scan.tcnt;
  a.rcap = cap;
  a.hit_s = ix->range.s;
  a.hit_i = ix->range.i;
  HIPCHK(launch_sq_range_scan(a, st));
  return 0;
}

const ThrPass& sq8_thr_pass() {
  static const ThrPass P = {
    "flat SQ8",
    [](const knnx_index* ix) { return ix->fsq.on; },
    [](knnx_index* ix) -> ThrState& { return ix->fsq.thr_scan; },
    sq8_pass_max,
    sq8_front,
    sq8_pass_top64,
    sq8_pass_probed_rows,
    sq8_pass_launch_threshold,
  };
  return P;
}

int sq8_refuse_unless_thr(const knnx_index* ix, const std::string& who) { return ix && ix->fsq.on && ix->fsq.thr_scan.on ? 0 : sq8_refuse(ix, who); }

extern "C" int knnx_sq8_set_threshold_scan(knnx_index* ix, int on) { return thr_set_switch(ix, sq8_thr_pass(), on); }
extern "C" int knnx_sq8_threshold_scan(const knnx_index* ix) { return thr_switch(ix, sq8_thr_pass()); }
extern "C" int knnx_sq8_threshold_stats(knnx_index* ix, int64_t* queries, int64_t* launches, int64_t* query_scans, int64_t* hits) {
  return thr_stats(ix, sq8_thr_pass(), queries, launches, query_scans, hits);
}

int sq8_decode_rows(knnx_index* ix, const int64_t* ids_dev, int64_t n, float* out_dev, hipStream_t st) {
  HIPCHK(launch_sq_decode_flat(ix->fsq.codes, ix->d, ix->fsq.vmin, ix->fsq.step, ix->id_base, ix->ntotal, ids_dev, n, out_dev, st));
  return KNNX_OK;
}

// ---- the quantiser ---------------------------------------------------------------------------------------------------------------
extern "C" int knnx_sq8_set_quantizer(knnx_index* ix, const float* vmin, const float* vdiff) {
  if (!ix || !vmin || !vdiff) return fail(KNNX_E_ARG, "bad sq8_set_quantizer arguments");
  const int d = ix->d;
  for (int j = 0; j < d; ++j)
    if (!isfinite(vmin[j]) || !isfinite(vdiff[j]) || vdiff[j] < 0.f)
      return fail(KNNX_E_ARG, "flat SQ8 needs finite vmin and finite vdiff >= 0 (column " + std::to_string(j) + ")");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (ix->pq.m || ix->sq.on || ix->ivf_nlist || ix->ivfb.nlist || ix->rows.borrowed || ix->rows || ix->ntotal != 0 || ix->fsq.on)
    return fail(KNNX_E_STATE, "the flat SQ8 quantizer is set once, on an empty index that is not an IVF index");
  if (set_dev(ix)) return KNNX_E_HIP;
  // scale and step in fp32 with IEEE division, here on the host (the IVF-SQ8 contract)
  std::vector<float> scale((size_t)d), step((size_t)d);
  for (int j = 0; j < d; ++j) {
    const float vd = vdiff[j];
    scale[j] = vd == 0.f ? 0.f : 255.f / vd;
    step[j] = vd / 255.f;
  }
  Sq8Flat f;
  hipError_t e = hipSuccess;
  dev_alloc(e, f.vmin, (size_t)d);
  dev_alloc(e, f.scale, (size_t)d);
  dev_alloc(e, f.step, (size_t)d);
  if (e == hipSuccess) e = hipMemcpy(f.vmin, vmin, (size_t)d * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(f.scale, scale.data(), (size_t)d * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(f.step, step.data(), (size_t)d * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP, std::string("sq8_set_quantizer: ") + hipGetErrorString(e));
  }
  f.vmin_h.assign(vmin, vmin + d);
  f.vdiff_h.assign(vdiff, vdiff + d);
  f.on = true;
  ix->fsq = std::move(f);
  ix->capacity = 0;
  ix->i8_ok = 0;  // (no fp16 rows: the int8 stage has nothing to copy)
  return KNNX_OK;
}

extern "C" int knnx_sq8_get_quantizer(knnx_index* ix, float* vmin, float* vdiff) {
  if (!ix || !vmin || !vdiff) return fail(KNNX_E_ARG, "bad sq8_get_quantizer arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->fsq.on) return fail(KNNX_E_STATE, "not a flat SQ8 index");
  memcpy(vmin, ix->fsq.vmin_h.data(), (size_t)ix->d * sizeof(float));
  memcpy(vdiff, ix->fsq.vdiff_h.data(), (size_t)ix->d * sizeof(float));
  return KNNX_OK;
}

extern "C" int knnx_sq8(const knnx_index* ix) { return ix && ix->fsq.on ? 1 : 0; }

// ---- codes in and out (host, id order) -------------------------------------------------------------------------------------------
static int sq8_copy_codes(knnx_index* ix, uint8_t* host, int64_t row0, int64_t n, bool to_device) {
  const int64_t chunk = std::max<int64_t>(1, (int64_t)(64u << 20) / ix->d);
  int r = ensure_pin(ix, (size_t)std::min(chunk, n) * ix->d);
  if (r) return r;
  for (int64_t o = 0; o < n; o += chunk) {
    const int64_t m = std::min(chunk, n - o);
    const size_t bytes = (size_t)m * ix->d;
    uint8_t* dev = ix->fsq.codes + (size_t)(row0 + o) * ix->d;
    if (to_device) {
      memcpy(ix->pin.p, host + (size_t)o * ix->d, bytes);
      HIPCHK(hipMemcpyAsync(dev, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->stream));
      HIPCHK(hipStreamSynchronize(ix->stream));
    } else {
      HIPCHK(hipMemcpyAsync(ix->pin.p, dev, bytes, hipMemcpyDeviceToHost, ix->stream));
      HIPCHK(hipStreamSynchronize(ix->stream));
      memcpy(host + (size_t)o * ix->d, ix->pin.p, bytes);
    }
  }
  return KNNX_OK;
}

extern "C" int knnx_sq8_add_codes(knnx_index* ix, const uint8_t* codes, int64_t n) {
  if (!ix || (!codes && n > 0) || n < 0) return fail(KNNX_E_ARG, "bad sq8_add_codes arguments");
  if (n == 0) return KNNX_OK;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->fsq.on) return fail(KNNX_E_STATE, "not a flat SQ8 index (knnx_sq8_set_quantizer first)");
  if (set_dev(ix)) return KNNX_E_HIP;
  int r = sq8_grow_for(ix, n);
  if (r) return r;
  if ((r = sq8_copy_codes(ix, const_cast<uint8_t*>(codes), ix->ntotal, n, true))) return r;
  ix->ntotal += n;
  return KNNX_OK;
}

extern "C" int knnx_sq8_get_codes(knnx_index* ix, uint8_t* codes) {
  if (!ix || !codes) return fail(KNNX_E_ARG, "bad sq8_get_codes arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->fsq.on) return fail(KNNX_E_STATE, "not a flat SQ8 index");
  if (ix->ntotal == 0) return KNNX_OK;
  if (set_dev(ix)) return KNNX_E_HIP;
  return sq8_copy_codes(ix, codes, 0, ix->ntotal, false);
}
