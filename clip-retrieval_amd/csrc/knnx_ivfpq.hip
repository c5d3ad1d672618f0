// knnx_ivfpq.hip -- IVF-PQ on the host side: the search pass, the quantiser and code entry points, codebook training
// (knnx_pqb_*) (see knnx_host.h; kernels in knn_pq_kernels.hip).

#include "knnx_host.h"
#include "knnx_pq_plan.h"
#include "knnx_rot_shape.h"

// ---------------------------------------------------------------------------------------------
// IVF-PQ pass of 1 .. 256 queries already in HBM (csrc/knn_pq_kernels.hip): the coarse quantiser of the multi-block IVF pass
// (one score dump over the centroids + the radix select of ivf_select_mark_kernel: the nprobe largest <q, c>, ties to the lower
// list id), the probed lists of every query, its lookup table, the ADC list scan, the merge of the per-workgroup lists.
// ---------------------------------------------------------------------------------------------
//
// The front half of a pass, shared by the top-k pass and the threshold passes: rotation, query prep, coarse dump, select / mark,
// probe lists and lookup tables.  Leaves probe / pscore / pcnt / lut of the nq queries in ix->pqs, and in ix->pqs.np the lists probed
// per query.
static int pq_front(knnx_index* ix, const float* q_dev, int nq, hipStream_t st) {
  const int np = std::min(ix->ivf_nprobe, ix->ivf_nlist);
  const int dq = pq_dq(ix);  // everything behind the rotation is dq wide (= d unless the index was given a d_out)
  HIPCHK(ix->pqs.alloc(dq, (size_t)ix->ivf_nlist, ix->pq.m, np));
  knnx_index* c = ix->cent;
  const int nblk = (nq + KNN_NQ - 1) / KNN_NQ;
  if (ix->pq.rot) {  // OPQ: everything below sees q' = A q
    if (!ix->pqs.qrot) HIPCHK(ix->pqs.qrot.alloc((size_t)PQ_PASS * dq));
    HIPCHK(launch_rot_queries(ix->pq.rot, ix->d, dq, q_dev, nq, ix->pqs.qrot, st));
    q_dev = ix->pqs.qrot;
  }
  HIPCHK(launch_prep_blocks(q_dev, nq, dq, ix->pqs.qfrag, ix->pqs.thr, ix->pqs.thr + PQ_PASS, st));
  ScanArgs ca{};
  ca.X = c->rows;
  ca.N = c->ntotal;
  ca.d = c->d;
  ca.qfrag = ix->pqs.qfrag;
  ca.nq = nq;
  ca.grid = std::max(1, ix->n_cu / nblk) * nblk;
  ca.thr_g = ix->pqs.thr;
  ca.nblk = nblk;
  ca.k = 1;
  ca.cap = 2;
  ca.mode = 2;
  ca.range_cap = (unsigned)ix->ivf_nlist;
  ca.range_s = ix->pqs.scores;
  HIPCHK(launch_scan(ca, st));
  HIPCHK(launch_ivf_select_mark(ix->pqs.scores, nq, np, ix->ivf_nlist, ix->pqs.masks, st));
  HIPCHK(launch_pq_probe(ix->pqs.masks, ix->pqs.scores, nq, ix->ivf_nlist, np, ix->pqs.pcnt, ix->pqs.probe, ix->pqs.pscore, st));
  if (ix->pq.m == 256) {  // the two-half scan: where every probe's rows start in its query's slab of partial sums
    HIPCHK(launch_pq_probe_offsets(ix->pqs.probe, ix->pqs.pcnt, np, ix->ivf.size, ix->pqs.poff, nq, st));
    ix->pqs.half_nq = 0;  // the sums of an earlier front half are not these queries'
  }
  HIPCHK(launch_pq_lut(q_dev, nq, dq, ix->pq.m, ix->pq.cb, ix->pqs.lut, st));
  ix->pqs.np = np;
  return 0;
}

// shares a query's probed lists are split into (workgroups per query of the ADC scans)
static int pq_nsplit(int np, int nq) { return std::max(1, std::min(std::min(np, PQ_MAX_SPLIT), (PQ_TARGET_WG + nq - 1) / nq)); }

// ---------------------------------------------------------------------------------------------
// M = 256: the ADC stage in two halves of m (knn_pq_kernels.hip; sizes: knnx_pq_plan.h).  What the stage is asked for:
// ---------------------------------------------------------------------------------------------
struct PqStage {
  enum Kind { TOPK, CAND, RANGE } kind = TOPK;
  int k = 0;                   // TOPK: k <= 64; CAND: kc
  float* part_s = nullptr;     // TOPK / CAND: the partial lists of the nsplit x nq workgroups
  uint32_t* part_i = nullptr;
  const float* thr = nullptr;  // RANGE: thresholds [nq], counters [nq] (cleared here), pool slices of cap hits
  unsigned* cnt = nullptr;
  unsigned cap = 0;
  float* hit_s = nullptr;
  uint32_t* hit_r = nullptr;
};

// S of the index at np probed lists (host arithmetic; cached until nprobe changes or the index is rebuilt)
static uint64_t pq_slab(knnx_index* ix, int np) {
  if (ix->pq.slab_np != np) {
    ix->pq.slab = pq_plan_slab(ix->pq.size_h.data(), (int64_t)ix->pq.size_h.size(), np);
    ix->pq.slab_np = np;
  }
  return ix->pq.slab;
}

// the buffer of plan.floats() partial sums (at least one), grown on demand
static int pq_half_buffer(knnx_index* ix, const PqPlan& plan) {
  PqScratch& S = ix->pqs;
  const uint64_t need = std::max<uint64_t>(plan.floats(), 1);
  if (S.half && S.half_cap >= need) return 0;
  S.half.reset();
  S.half_cap = 0;
  S.half_nq = 0;
  if (need > (uint64_t)SIZE_MAX / 4 || malloc_or_reclaim(ix, S.half, (size_t)need) != hipSuccess) {
    (void)hipGetLastError();
    return fail(KNNX_E_NOMEM, "IVF-PQ with M = 256: no device memory for " + std::to_string(need * 4) + " bytes of partial sums (" +
                                  std::to_string(plan.g) + " queries x " + std::to_string(plan.slab) +
                                  " probed rows x 4; KNNX_PQ_PARTIAL_MAX_BYTES lowers it)");
  }
  S.half_cap = need;
  return 0;
}

// The stage over the nq queries of the pass whose front half is in ix->pqs: per sub-group of the plan the lower-half kernel, then the
// upper half of the scan asked for.  A pass that is ONE sub-group keeps its partial sums for the later stages of the same front half
// (the k = 64 pass and every threshold scan of a descent read the same sums); pq_front forgets them.
static int pq_two_half_stage(knnx_index* ix, int nq, int np, int nsplit, const PqStage& a, hipStream_t st) {
  PqScratch& S = ix->pqs;
  const PqPlan plan(pq_slab(ix, np), nq, ix->pq.partial_budget);
  int r = pq_half_buffer(ix, plan);
  if (r) return r;
  if (a.kind == PqStage::RANGE) HIPCHK(hipMemsetAsync(a.cnt, 0, (size_t)nq * sizeof(unsigned), st));
  const bool whole = plan.groups() == 1;
  for (int i = 0; i < plan.groups(); ++i) {
    const int q0 = plan.first(i), g = plan.count(i);
    if (!(whole && S.half_nq == nq)) {
      // (with kept sums a query may have finished since they were made: only a scan that makes its own may skip the finished ones)
      HIPCHK(launch_pq_adc_lower(ix->pq.codes, S.lut, S.probe, S.pcnt, np, pq_nsplit(np, g), ix->ivf.tile0, ix->ivf.size, S.poff,
                                 whole ? nullptr : a.thr, (size_t)plan.slab, q0, g, S.half, st));
      S.half_nq = whole ? nq : 0;
    }
    switch (a.kind) {
      case PqStage::TOPK:
        HIPCHK(launch_pq_adc_upper(ix->pq.codes, S.lut, S.probe, S.pscore, S.pcnt, np, nsplit, ix->ivf.tile0, ix->ivf.size, ix->ivf.idmap, a.k,
                                   nq, a.part_s, a.part_i, S.part_n, S.half, S.poff, (size_t)plan.slab, q0, g, st));
        break;
      case PqStage::CAND:
        HIPCHK(launch_pq_cand_upper(ix->pq.codes, S.lut, S.probe, S.pscore, S.pcnt, np, nsplit, ix->ivf.tile0, ix->ivf.size, ix->ivf.idmap, a.k,
                                    nq, a.part_s, a.part_i, S.part_n, S.half, S.poff, (size_t)plan.slab, q0, g, st));
        break;
      case PqStage::RANGE:
        HIPCHK(launch_pq_range_upper(ix->pq.codes, S.lut, S.probe, S.pscore, S.pcnt, np, nsplit, ix->ivf.tile0, ix->ivf.size, a.thr, a.cnt,
                                     a.cap, a.hit_s, a.hit_r, S.half, S.poff, (size_t)plan.slab, q0, g, st));
        break;
    }
  }
  return 0;
}

// the ADC top-k scan of the pass (k <= 64) into the partial lists part_s / part_i / S.part_n: one launch, or the two halves at M = 256
static int pq_stage_topk(knnx_index* ix, int nq, int np, int nsplit, int k, float* part_s, uint32_t* part_i, hipStream_t st) {
  PqScratch& S = ix->pqs;
  if (ix->pq.m == 256) {
    PqStage a;
    a.kind = PqStage::TOPK, a.k = k, a.part_s = part_s, a.part_i = part_i;
    return pq_two_half_stage(ix, nq, np, nsplit, a, st);
  }
  HIPCHK(launch_pq_adc_scan(ix->pq.codes, ix->pq.m, S.lut, S.probe, S.pscore, S.pcnt, np, nsplit, ix->ivf.tile0, ix->ivf.size, ix->ivf.idmap, k, nq,
                            part_s, part_i, S.part_n, st));
  return 0;
}

// Refine store (knnx_ivfpq_set_refine): the ADC stage keeps kc = k x k_factor candidates instead of k -- for kc <= 64 the scan and
// merge above, for more the workgroup-queue scan and the LDS selection (pq_cand_scan_kernel, pq_cand_select_kernel) with the
// shares capped so that shares x kc <= PQ_SEL_MAX -- and the candidates are re-scored from the fp16 rows with the ORIGINAL query
// (pq_rescore_kernel) and ranked (pq_refine_topk_kernel).
int scan_topk_pq(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st) {
  if (nq < 1 || nq > PQ_PASS || k < 1 || k > KNNX_MAX_K_FAST || !ix->cent || !ix->ivf_nlist)
    return fail(KNNX_E_STATE, "internal: IVF-PQ pass misuse");
  const int kc = ix->pq.refine ? k * ix->pq.k_factor : k;
  if (kc > PQ_REFINE_MAX)
    return fail(KNNX_E_ARG, "k x k_factor = " + std::to_string(k) + " x " + std::to_string(ix->pq.k_factor) + " exceeds " +
                                std::to_string(PQ_REFINE_MAX) + " candidates per query");
  const float* q_orig = q_dev;
  int r = pq_front(ix, q_orig, nq, st);
  if (r) return r;
  const int np = ix->pqs.np;
  if (ix->pq.refine) HIPCHK(ix->pqs.alloc_refine());
  int nsplit = pq_nsplit(np, nq);
  if (ix->pq.refine) {
    PqScratch& S = ix->pqs;
    HIPCHK(ix->prof.begin(ix->prof.on, st));
    if (kc <= PQ_MAX_K) {
      if ((r = pq_stage_topk(ix, nq, np, nsplit, kc, S.part_s, S.part_i, st))) return r;
      HIPCHK(launch_merge_u32(S.part_s, S.part_i, S.part_n, nsplit, nq, kc, nq, kc, ix->id_base, ix->ivf.idmap, S.rdc, S.rcand, nullptr, st));
    } else {
      nsplit = std::max(1, std::min(nsplit, PQ_SEL_MAX / kc));
      if (ix->pq.m == 256) {
        PqStage a;
        a.kind = PqStage::CAND, a.k = kc, a.part_s = S.rpart_s, a.part_i = S.rpart_r;
        if ((r = pq_two_half_stage(ix, nq, np, nsplit, a, st))) return r;
      } else {
        HIPCHK(launch_pq_cand_scan(ix->pq.codes, ix->pq.m, S.lut, S.probe, S.pscore, S.pcnt, np, nsplit, ix->ivf.tile0, ix->ivf.size,
                                   ix->ivf.idmap, kc, nq, S.rpart_s, S.rpart_r, S.part_n, st));
      }
      HIPCHK(launch_pq_cand_select(S.rpart_s, S.rpart_r, S.part_n, nsplit, nq, kc, ix->ivf.idmap, S.rcand, st));
    }
    HIPCHK(launch_pq_refine(ix->rows, ix->d, q_orig, nq, ix->id_base, ix->ntotal, ix->ivf.inv, S.rcand, kc, k, S.rscore, D_out, I_out, st));
    HIPCHK(ix->prof.end(ix->prof.on, st));
    return 0;
  }
  HIPCHK(ix->prof.begin(ix->prof.on, st));
  if ((r = pq_stage_topk(ix, nq, np, nsplit, k, ix->pqs.part_s, ix->pqs.part_i, st))) return r;
  HIPCHK(ix->prof.end(ix->prof.on, st));
  HIPCHK(launch_merge_u32(ix->pqs.part_s, ix->pqs.part_i, ix->pqs.part_n, nsplit, nq, k, nq, k, ix->id_base, ix->ivf.idmap, D_out, I_out,
                          nullptr, st));
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Threshold passes (the switch knnx_ivfpq_set_threshold_scan; knnx_range.hip drives them): after pq_front, any number of
// pq_range_scan_kernel launches over the same probe lists and lookup tables with new per-query thresholds.
// ---------------------------------------------------------------------------------------------
// the plain ADC top-64 scores of the pass whose front half is in ix->pqs (no refine stage) -> D64 host [nq][64], -FLT_MAX padded.
// Synchronises.
static int pq_pass_top64(knnx_index* ix, int nq, float* D64, hipStream_t st) {
  PqScratch& S = ix->pqs;
  const int np = S.np, nsplit = pq_nsplit(np, nq), k = KNNX_MAX_K_FAST;
  int r = pq_stage_topk(ix, nq, np, nsplit, k, S.part_s, S.part_i, st);
  if (r) return r;
  HIPCHK(launch_merge_u32(S.part_s, S.part_i, S.part_n, nsplit, nq, k, nq, k, ix->id_base, ix->ivf.idmap, ix->flat.D_dev, ix->flat.I_dev,
                          nullptr, st));
  HIPCHK(hipMemcpyAsync(D64, ix->flat.D_dev, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// rows in the probed lists of every query of the pass -> total [nq].  Synchronises.
static int pq_pass_probed_rows(knnx_index* ix, int nq, std::vector<int64_t>& total, hipStream_t st) {
  const int np = ix->pqs.np;
  std::vector<unsigned> pc((size_t)nq);
  std::vector<int> pr((size_t)nq * np);
  HIPCHK(hipMemcpyAsync(pc.data(), ix->pqs.pcnt, pc.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(pr.data(), ix->pqs.probe, pr.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  total.assign((size_t)nq, 0);
  for (int q = 0; q < nq; ++q)
    for (int p = 0; p < std::min<int>((int)pc[q], np); ++p) {
      const int l = pr[(size_t)q * np + p];
      if (l < 0 || l >= ix->ivf_nlist || (size_t)l >= ix->pq.size_h.size()) return fail(KNNX_E_STATE, "internal: probe list out of range");
      total[q] += ix->pq.size_h[l];
    }
  return 0;
}

// the threshold ADC scan of the pass (ThrPass::launch_threshold); +INFINITY skips a query
static int pq_pass_launch_threshold(knnx_index* ix, int nq, unsigned cap, hipStream_t st) {
  PqScratch& S = ix->pqs;
  ThrState& T = ix->pq.thr;
  const int np = S.np;
  if (ix->pq.m == 256) {
    PqStage a;
    a.kind = PqStage::RANGE, a.thr = T.tthr, a.cnt = T.tcnt, a.cap = cap, a.hit_s = ix->range.s, a.hit_r = ix->range.i;
    return pq_two_half_stage(ix, nq, np, pq_nsplit(np, nq), a, st);
  }
  HIPCHK(launch_pq_range_scan(ix->pq.codes, ix->pq.m, S.lut, S.probe, S.pscore, S.pcnt, np, pq_nsplit(np, nq), ix->ivf.tile0, ix->ivf.size,
                              T.tthr, T.tcnt, cap, ix->range.s, ix->range.i, nq, st));
  return 0;
}

// (a function-local table: a namespace-scope constant would be emitted for the device too, where the host functions it names do not exist)
const ThrPass& pq_thr_pass() {
  static const ThrPass P = {
    "IVF-PQ",
    [](const knnx_index* ix) { return ix->pq.m != 0; },
    [](knnx_index* ix) -> ThrState& { return ix->pq.thr; },
    [](const knnx_index*) { return PQ_PASS; },
    pq_front,
    pq_pass_top64,
    pq_pass_probed_rows,
    pq_pass_launch_threshold,
  };
  return P;
}

extern "C" int knnx_ivfpq_set_threshold_scan(knnx_index* ix, int on) { return thr_set_switch(ix, pq_thr_pass(), on); }
extern "C" int knnx_ivfpq_threshold_scan(const knnx_index* ix) { return thr_switch(ix, pq_thr_pass()); }
extern "C" int knnx_ivfpq_threshold_stats(knnx_index* ix, int64_t* queries, int64_t* launches, int64_t* query_scans, int64_t* hits) {
  return thr_stats(ix, pq_thr_pass(), queries, launches, query_scans, hits);
}

// ---------------------------------------------------------------------------------------------
// IVF-PQ (faiss IndexIVFPQ(IndexFlatIP(d), d, nlist, M, 8), METRIC_INNER_PRODUCT, by_residual): the index type autofaiss picks
// for large corpora (the reference's notebook builds OPQ256_768,IVF16384_HNSW32,PQ256x8).  The quantizer is set on an empty
// index; the IVF build protocol then ENCODES rows into the list-sorted arena; searches go through scan_topk_pq.
// ---------------------------------------------------------------------------------------------
static const char* const PQ_M_RULE = "IVF-PQ needs M in {16, 32, 64, 128} dividing d (8-bit codes), or M = 256 with d >= 512";

extern "C" int knnx_ivfpq_set_quantizer(knnx_index* ix, int M, const float* codebooks) {
  if (!ix || !codebooks) return fail(KNNX_E_ARG, "bad ivfpq_set_quantizer arguments");
  const int dq = pq_dq(ix);  // (the rule speaks of the quantiser width: d_out where knnx_ivfpq_set_out_dim gave one)
  if (!pq_supported(dq, M)) return fail(KNNX_E_ARG, PQ_M_RULE);
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (ix->sq.on) return fail(KNNX_E_STATE, "the PQ quantizer cannot be set on an IVF-SQ8 index");
  if (ix->rows.borrowed || ix->ntotal != 0 || ix->ivf_nlist || ix->ivfb.nlist || ix->pq.m)
    return fail(KNNX_E_STATE, "the PQ quantizer is set once, on an empty index, before knnx_ivf_begin");
  const size_t bytes = (size_t)256 * dq * sizeof(float);
  HIPCHK(ix->pq.cb.alloc((size_t)256 * dq));
  HIPCHK(hipMemcpy(ix->pq.cb, codebooks, bytes, hipMemcpyHostToDevice));
  ix->pq.m = M;
  if (M == 256) {  // the budget of the two-half scan's partial sums, read once like the switches of knnx_create
    const char* v = getenv("KNNX_PQ_PARTIAL_MAX_BYTES");
    const long long b = (v && v[0]) ? atoll(v) : 0;
    ix->pq.partial_budget = b > 0 ? (uint64_t)b : PQ_PARTIAL_DEFAULT_BYTES;
  }
  return KNNX_OK;
}

extern "C" int knnx_ivfpq_m(const knnx_index* ix) { return ix ? ix->pq.m : 0; }

// ---- the quantiser width (faiss OPQMatrix(d_in, M, d_out) with d_out > d_in): chosen before the quantizer, which is d_out wide ------
extern "C" int knnx_ivfpq_set_out_dim(knnx_index* ix, int d_out) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  if (d_out != ix->d && !rot_shape_supported(ix->d, d_out))
    return fail(KNNX_E_ARG, "d_out = " + std::to_string(d_out) + " on an index of d = " + std::to_string(ix->d) +
                                ": both widths must be multiples of 256 with 256 <= d <= d_out <= 1024");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (ix->pq.m || ix->rows.borrowed || ix->ntotal != 0 || ix->ivf_nlist || ix->ivfb.nlist)
    return fail(KNNX_E_STATE, "d_out is chosen on an empty index, before knnx_ivfpq_set_quantizer");
  ix->pq.dq = d_out == ix->d ? 0 : d_out;
  return KNNX_OK;
}
extern "C" int knnx_ivfpq_out_dim(const knnx_index* ix) { return ix && ix->pq.m ? pq_dq(ix) : 0; }

// ---- refine store (faiss IndexRefineFlat(IndexIVFPQ)): the index keeps the fp16 rows next to the codes --------------------------
extern "C" int knnx_ivfpq_set_refine(knnx_index* ix, int on) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->pq.m || ix->ntotal != 0 || ix->ivf_nlist || ix->ivfb.nlist)
    return fail(KNNX_E_STATE, "the refine store is chosen on an IVF-PQ index after knnx_ivfpq_set_quantizer and before knnx_ivf_begin");
  ix->pq.refine = on != 0;
  return KNNX_OK;
}
extern "C" int knnx_ivfpq_refine(const knnx_index* ix) { return ix && ix->pq.refine ? 1 : 0; }

extern "C" int knnx_ivfpq_set_k_factor(knnx_index* ix, int k_factor) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  if (k_factor < 1 || k_factor > PQ_REFINE_MAX) return fail(KNNX_E_ARG, "k_factor must lie in 1 .. " + std::to_string(PQ_REFINE_MAX));
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->pq.m) return fail(KNNX_E_STATE, "not an IVF-PQ index");
  ix->pq.k_factor = k_factor;
  return KNNX_OK;
}
extern "C" int knnx_ivfpq_k_factor(const knnx_index* ix) { return ix ? ix->pq.k_factor : 0; }

// bytes of the code arena and of the row arena (0 without a refine store) of an IVF-PQ index
extern "C" int knnx_ivfpq_arena_bytes(knnx_index* ix, int64_t* code_bytes, int64_t* row_bytes) {
  if (!ix || !code_bytes || !row_bytes) return fail(KNNX_E_ARG, "bad ivfpq_arena_bytes arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->pq.m) return fail(KNNX_E_STATE, "not an IVF-PQ index");
  *code_bytes = ix->pq.codes ? ix->capacity * (int64_t)ix->pq.m : 0;
  *row_bytes = ix->pq.refine && ix->rows ? ix->capacity * (int64_t)ix->d * 2 : 0;
  return KNNX_OK;
}

// ---- OPQ rotation (faiss IndexPreTransform(OPQMatrix(d, M, d_out), IndexIVFPQ)) --------------------------------------------------
// A f32 [d_out][d] row-major, y = A x.  Orthonormal or refused, checked in float64 on the host (csrc/knnx_rot_shape.h; at most 1e9
// multiply-adds, once per index): the square matrix by its rows, max |A A^T - I| <= 1e-3; the rectangular one (d_out > d) by its
// columns, max |A^T A - I_d| <= 1e-3 -- its rows cannot be orthonormal, its columns are what keeps <A q, A x> = <q, x>.
extern "C" int knnx_ivfpq_set_rotation(knnx_index* ix, const float* A) {
  if (!ix || !A) return fail(KNNX_E_ARG, "bad ivfpq_set_rotation arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (!ix->pq.m || ix->ntotal != 0 || ix->ivf_nlist || ix->ivfb.nlist)
    return fail(KNNX_E_STATE, "the rotation is set on an IVF-PQ index after knnx_ivfpq_set_quantizer and before knnx_ivf_begin");
  const int d = ix->d, dq = pq_dq(ix);
  if (dq == d) {
    if (!(rot_row_gram_error(A, d, d) <= 1e-3)) return fail(KNNX_E_ARG, "the rotation is not orthonormal (max |A A^T - I| > 1e-3)");
  } else {
    std::vector<double> G((size_t)d * d);
    if (!(rot_col_gram_error(A, dq, d, G.data()) <= 1e-3))
      return fail(KNNX_E_ARG, "the rotation [" + std::to_string(dq) + "][" + std::to_string(d) +
                                  "] does not have orthonormal columns (max |A^T A - I| > 1e-3)");
  }
  hipError_t e = hipSuccess;
  dev_alloc(e, ix->pq.rot, (size_t)dq * d);
  dev_alloc(e, ix->pq.rot_w, (size_t)2 * dq * d);
  if (e == hipSuccess) e = hipMemcpy(ix->pq.rot, A, (size_t)dq * d * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_rot_split(ix->pq.rot, d, dq, ix->pq.rot_w, ix->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
  if (e != hipSuccess) {
    ix->pq.rot.reset();
    ix->pq.rot_w.reset();
    ix->pq.rot_h.clear();
    HIPCHK(e);
  }
  ix->pq.rot_h.assign(A, A + (size_t)dq * d);
  return KNNX_OK;
}

// 0 and the matrix [d_out][d], or 1 (A untouched) when the index has no rotation
extern "C" int knnx_ivfpq_get_rotation(knnx_index* ix, float* A) {
  if (!ix || !A) return fail(KNNX_E_ARG, "bad ivfpq_get_rotation arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (ix->pq.rot_h.empty()) return 1;
  memcpy(A, ix->pq.rot_h.data(), ix->pq.rot_h.size() * sizeof(float));
  return KNNX_OK;
}

// The stand-alone row rotation: out[i] = fp16(A rows[i]) for n fp16 rows in HBM (the OPQ trainer, the device-streamed build's
// assignment pass).  A: host f32 [d_out][d_in] (not checked for orthonormality: the trainer's iterates are what they are); rows are
// d_in wide, out rows d_out wide; out must not overlap rows.  Synchronous.
static int rotate_rows_device(int device, const float* A_host, const void* rows_dev_f16, int64_t n, int d, int dq, void* out_dev_f16,
                              void* stream) {
  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  DevBuf<float> A;
  DevBuf<_Float16> W;
  HIPCHK(A.alloc((size_t)dq * d));
  HIPCHK(W.alloc((size_t)2 * dq * d));
  HIPCHK(hipMemcpyAsync(A, A_host, (size_t)dq * d * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(launch_rot_split(A, d, dq, W, st));
  for (int64_t o = 0; o < n; o += IVFB_CHUNK)
    HIPCHK(launch_rotate_f16(W, d, dq, (const _Float16*)rows_dev_f16 + (size_t)o * d, std::min(IVFB_CHUNK, n - o),
                             (_Float16*)out_dev_f16 + (size_t)o * dq, st));
  HIPCHK(hipStreamSynchronize(st));
  return KNNX_OK;
}

extern "C" int knnx_rotate_f16_device(int device, const float* A_host, const void* rows_dev_f16, int64_t n, int d, void* out_dev_f16,
                                      void* stream) {
  if (!A_host || (n > 0 && (!rows_dev_f16 || !out_dev_f16)) || n < 0) return fail(KNNX_E_ARG, "bad rotate_f16_device arguments");
  if (d != 256 && d != 512 && d != 768 && d != 1024) return fail(KNNX_E_ARG, "the rotation takes d in {256, 512, 768, 1024}");
  if (n == 0) return KNNX_OK;
  return rotate_rows_device(device, A_host, rows_dev_f16, n, d, d, out_dev_f16, stream);
}

extern "C" int knnx_rotate_rect_f16_device(int device, const float* A_host, const void* rows_dev_f16, int64_t n, int d_in, int d_out,
                                           void* out_dev_f16, void* stream) {
  if (!A_host || (n > 0 && (!rows_dev_f16 || !out_dev_f16)) || n < 0) return fail(KNNX_E_ARG, "bad rotate_rect_f16_device arguments");
  if (!rot_shape_supported(d_in, d_out))
    return fail(KNNX_E_ARG, "the rotation takes d_in <= d_out, both in {256, 512, 768, 1024} (got d_in = " + std::to_string(d_in) +
                                ", d_out = " + std::to_string(d_out) + ")");
  if (n == 0) return KNNX_OK;
  return rotate_rows_device(device, A_host, rows_dev_f16, n, d_in, d_out, out_dev_f16, stream);
}

// G = X^T Y (f32 [d][d], device) for fp16 rows X and f32 rows Y [n][d] in HBM: the d x d product of an OPQ iteration, every element
// one fp32 sum over the rows in ascending order.  Synchronous.
extern "C" int knnx_xty_device(int device, const void* x_dev_f16, const float* y_dev_f32, int64_t n, int d, float* g_dev, void* stream) {
  if (!x_dev_f16 || !y_dev_f32 || !g_dev || n <= 0) return fail(KNNX_E_ARG, "bad xty_device arguments");
  if (d != 256 && d != 512 && d != 768 && d != 1024) return fail(KNNX_E_ARG, "xty takes d in {256, 512, 768, 1024}");
  HIPCHK(hipSetDevice(device));
  HIPCHK(launch_xty((const _Float16*)x_dev_f16, y_dev_f32, n, d, g_dev, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return KNNX_OK;
}

int pq_decode_rows(knnx_index* ix, const int64_t* ids_dev, int64_t n, float* out_dev, hipStream_t st) {
  if (ix->pq.refine) {  // the stored rows, no decode and no back-rotation (faiss IndexRefine::reconstruct)
    HIPCHK(launch_gather_inv(ix->rows, ix->d, ix->id_base, ix->ntotal, ix->ivf.inv, ids_dev, n, out_dev, st));
    return KNNX_OK;
  }
  const int dq = pq_dq(ix);  // the decode is dq wide; A^T brings it back to d (without a rotation dq = d: knnx_ivf_begin saw to it)
  float* dec = out_dev;
  if (ix->pq.rot) {
    int r = ensure_scratch(ix, 5, (size_t)n * dq * sizeof(float), (void**)&dec);
    if (r) return r;
  }
  HIPCHK(launch_pq_decode(ix->pq.codes, dq, ix->pq.m, ix->pq.cb, ix->cent ? ix->cent->rows : nullptr, ix->ivf.tile0, ix->ivf_nlist,
                          ix->id_base, ix->ntotal, ix->ivf.inv, ids_dev, n, dec, st));
  if (ix->pq.rot) HIPCHK(launch_rot_back(ix->pq.rot, ix->d, dq, dec, n, out_dev, st));
  return KNNX_OK;
}

extern "C" int knnx_ivfpq_get_codebooks(knnx_index* ix, float* codebooks) {
  if (!ix || !codebooks) return fail(KNNX_E_ARG, "bad ivfpq_get_codebooks arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->pq.m) return fail(KNNX_E_STATE, "not an IVF-PQ index");
  if (set_dev(ix)) return KNNX_E_HIP;
  HIPCHK(hipMemcpy(codebooks, ix->pq.cb, (size_t)256 * pq_dq(ix) * sizeof(float), hipMemcpyDeviceToHost));
  return KNNX_OK;
}

// every row of a built index in arena order: ids [ntotal], lists [ntotal], codes [ntotal][M]
extern "C" int knnx_ivfpq_get_codes(knnx_index* ix, int64_t* ids, int32_t* lists, uint8_t* codes) {
  if (!ix || !ids || !lists || !codes) return fail(KNNX_E_ARG, "bad ivfpq_get_codes arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->pq.m || !ix->ivf_nlist) return fail(KNNX_E_STATE, "not a built IVF-PQ index (knnx_ivf_end first)");
  return ivf_export_codes_locked(ix, ix->pq.codes, ix->pq.m, ix->pq.tile0_h, ix->pq.size_h, "IVF-PQ", ids, lists, codes);
}

// precomputed codes [n][M] (host) into an index between knnx_ivf_begin and knnx_ivf_end (an index loaded from its saved codes)
extern "C" int knnx_ivfpq_add_codes(knnx_index* ix, const uint8_t* codes, int64_t n, const int64_t* ids, const int32_t* lists,
                                    const int32_t* pos) {
  if (!ix || (n > 0 && (!codes || !ids || !lists || !pos)) || n < 0) return fail(KNNX_E_ARG, "bad ivfpq_add_codes arguments");
  if (n == 0) return KNNX_OK;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (!ix->pq.m || !ix->ivfb.nlist) return fail(KNNX_E_STATE, "set the PQ quantizer and call knnx_ivf_begin first");
  if (ix->pq.refine) return fail(KNNX_E_STATE, "an index with a refine store takes rows (knnx_ivf_add_assigned), not codes: it has no rows to store");
  return ivf_import_codes_locked(ix, ix->pq.codes, ix->pq.m, codes, n, ids, lists, pos);
}

// ---- codebook training (faiss ProductQuantizer::train on the residuals of a sample; one L2 k-means of 256 per sub-quantiser) ----
struct knnx_pq_builder {
  int device = 0, d = 0, M = 0;
  Stream stream;
  DevBuf<float> cb;  // [M][256][d / M]
  // the sample (knnx_pqb_set_sample*): one group, replaced as a whole
  struct Sample {
    int nlist = 0;
    int64_t n = 0;
    DevBuf<_Float16> X;      // rows [n][d]; borrowed after knnx_pqb_set_sample_device
    DevBuf<int32_t> lists;   // [n] their lists
    DevBuf<_Float16> cent;   // [nlist][d]
    DevBuf<uint8_t> codes;   // [n][M]
    DevBuf<int32_t> order;   // [M][n]
    DevBuf<int32_t> off;     // [M][257]
  } s;
  std::vector<uint8_t> h_codes;
  std::vector<int32_t> h_order, h_off;
};

extern "C" void knnx_pqb_destroy(knnx_pq_builder* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  delete b;
}

extern "C" int knnx_pqb_create(int device, int d, int M, knnx_pq_builder** out) {
  if (!out) return fail(KNNX_E_ARG, "out is null");
  *out = nullptr;
  if (!pq_supported(d, M)) return fail(KNNX_E_ARG, PQ_M_RULE);
  HIPCHK(hipSetDevice(device));
  knnx_pq_builder* b = new knnx_pq_builder();
  b->device = device;
  b->d = d;
  b->M = M;
  hipError_t e = b->stream.create();
  dev_alloc(e, b->cb, (size_t)256 * d);
  if (e == hipSuccess) e = hipMemset(b->cb, 0, (size_t)256 * d * sizeof(float));
  if (e != hipSuccess) {
    knnx_pqb_destroy(b);
    return fail(e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP, std::string("pqb_create: ") + hipGetErrorString(e));
  }
  *out = b;
  return KNNX_OK;
}

// the part of set_sample shared by the host and the device variant: lists (host copy h_lists, validated), centroids, scratch
static int pqb_sample_common(knnx_pq_builder* b, int64_t n, const int32_t* h_lists, const uint16_t* centroids_f16, int nlist) {
  for (int64_t i = 0; i < n; ++i)
    if (h_lists[i] < 0 || h_lists[i] >= nlist) return fail(KNNX_E_ARG, "a sample row's list id is outside [0, nlist)");
  knnx_pq_builder::Sample& s = b->s;
  s.nlist = nlist;
  s.n = n;
  hipError_t e = hipSuccess;
  dev_alloc(e, s.lists, (size_t)n);
  dev_alloc(e, s.cent, (size_t)nlist * b->d);
  dev_alloc(e, s.codes, (size_t)n * b->M);
  dev_alloc(e, s.order, (size_t)n * b->M);
  dev_alloc(e, s.off, (size_t)b->M * 257);
  if (e == hipSuccess) e = hipMemcpy(s.lists, h_lists, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s.cent, centroids_f16, (size_t)nlist * b->d * sizeof(_Float16), hipMemcpyHostToDevice);
  if (e != hipSuccess) b->s = knnx_pq_builder::Sample();
  HIPCHK(e);
  return KNNX_OK;
}

extern "C" int knnx_pqb_set_sample(knnx_pq_builder* b, const uint16_t* rows_f16, const int32_t* lists, int64_t n, const uint16_t* centroids_f16,
                                   int nlist) {
  if (!b || !rows_f16 || !lists || !centroids_f16 || n <= 0 || n > INT32_MAX || nlist <= 0) return fail(KNNX_E_ARG, "bad pqb_set_sample arguments");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  b->s = knnx_pq_builder::Sample();
  HIPCHK(b->s.X.alloc((size_t)n * b->d));
  HIPCHK(hipMemcpy(b->s.X, rows_f16, (size_t)n * b->d * sizeof(_Float16), hipMemcpyHostToDevice));
  return pqb_sample_common(b, n, lists, centroids_f16, nlist);
}

// rows_dev: fp16 [n][d] borrowed (kept alive by the caller until the training is over); lists_dev: int32 [n] (copied)
extern "C" int knnx_pqb_set_sample_device(knnx_pq_builder* b, const void* rows_dev_f16, const int32_t* lists_dev, int64_t n,
                                          const uint16_t* centroids_f16, int nlist) {
  if (!b || !rows_dev_f16 || !lists_dev || !centroids_f16 || n <= 0 || n > INT32_MAX || nlist <= 0)
    return fail(KNNX_E_ARG, "bad pqb_set_sample_device arguments");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  b->s = knnx_pq_builder::Sample();
  std::vector<int32_t> h((size_t)n);
  HIPCHK(hipMemcpy(h.data(), lists_dev, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  b->s.X.borrow(rows_dev_f16);
  return pqb_sample_common(b, n, h.data(), centroids_f16, nlist);
}

// codebook entries mj[i] (= m * 256 + j) := residual sub-vector m of sample row sample_rows[i]
extern "C" int knnx_pqb_seed_from_sample(knnx_pq_builder* b, const int32_t* mj, const int64_t* sample_rows, int64_t n) {
  if (!b || (n > 0 && (!mj || !sample_rows)) || n < 0 || !b->s.X) return fail(KNNX_E_ARG, "bad pqb_seed_from_sample arguments (set a sample first)");
  if (n == 0) return KNNX_OK;
  for (int64_t i = 0; i < n; ++i)
    if (mj[i] < 0 || mj[i] >= b->M * 256 || sample_rows[i] < 0 || sample_rows[i] >= b->s.n) return fail(KNNX_E_ARG, "codebook entry / sample row out of range");
  HIPCHK(hipSetDevice(b->device));
  DevBuf<int32_t> mj_dev;
  DevBuf<int64_t> r_dev;
  HIPCHK(mj_dev.alloc((size_t)n));
  hipError_t e = r_dev.alloc((size_t)n);
  if (e == hipSuccess) e = hipMemcpy(mj_dev, mj, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(r_dev, sample_rows, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_pq_seed(b->s.X, b->d, b->M, b->s.lists, b->s.cent, mj_dev, r_dev, n, b->cb, b->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
  if (e != hipSuccess) return fail(KNNX_E_HIP, std::string("pqb_seed_from_sample: ") + hipGetErrorString(e));
  return KNNX_OK;
}

extern "C" int knnx_pqb_set_codebooks(knnx_pq_builder* b, const float* codebooks) {
  if (!b || !codebooks) return fail(KNNX_E_ARG, "bad pqb_set_codebooks arguments");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(b->cb, codebooks, (size_t)256 * b->d * sizeof(float), hipMemcpyHostToDevice));
  return KNNX_OK;
}

extern "C" int knnx_pqb_get_codebooks(knnx_pq_builder* b, float* codebooks) {
  if (!b || !codebooks) return fail(KNNX_E_ARG, "bad pqb_get_codebooks arguments");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(codebooks, b->cb, (size_t)256 * b->d * sizeof(float), hipMemcpyDeviceToHost));
  return KNNX_OK;
}

// One Lloyd iteration of the M k-means: encode the sample (argmin per sub-quantiser, ties -> smaller j) -> codes to the host ->
// counting sort per sub-quantiser (members ascending by sample row: the fixed summation order) -> mean update; an empty
// cluster keeps its centroid (the caller re-seeds it).  codes_out [n][M] (this iteration's assignment) and sizes_out [M][256]
// (host) may be null.
extern "C" int knnx_pqb_lloyd(knnx_pq_builder* b, uint8_t* codes_out, int64_t* sizes_out) {
  if (!b || !b->s.X) return fail(KNNX_E_ARG, "bad pqb_lloyd arguments (set a sample first)");
  HIPCHK(hipSetDevice(b->device));
  const int64_t n = b->s.n;
  const int M = b->M;
  b->h_codes.resize((size_t)n * M);
  b->h_order.resize((size_t)n * M);
  b->h_off.assign((size_t)M * 257, 0);
  HIPCHK(launch_pq_encode(b->s.X, n, b->d, M, b->s.lists, b->s.cent, b->cb, nullptr, nullptr, nullptr, 0, 0, 0, b->s.codes, nullptr, nullptr, b->stream));
  HIPCHK(hipMemcpyAsync(b->h_codes.data(), b->s.codes, (size_t)n * M, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  for (int m = 0; m < M; ++m) {
    int32_t* off = b->h_off.data() + (size_t)m * 257;
    for (int64_t i = 0; i < n; ++i) off[b->h_codes[(size_t)i * M + m] + 1]++;
    if (sizes_out)
      for (int j = 0; j < 256; ++j) sizes_out[(size_t)m * 256 + j] = off[j + 1];
    for (int j = 0; j < 256; ++j) off[j + 1] += off[j];
    std::vector<int32_t> cur(off, off + 256);
    int32_t* ord = b->h_order.data() + (size_t)m * n;
    for (int64_t i = 0; i < n; ++i) ord[cur[b->h_codes[(size_t)i * M + m]]++] = (int32_t)i;
  }
  if (codes_out) memcpy(codes_out, b->h_codes.data(), (size_t)n * M);
  HIPCHK(hipMemcpyAsync(b->s.order, b->h_order.data(), (size_t)n * M * sizeof(int32_t), hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->s.off, b->h_off.data(), (size_t)M * 257 * sizeof(int32_t), hipMemcpyHostToDevice, b->stream));
  HIPCHK(launch_pq_update(b->s.X, b->d, M, b->s.lists, b->s.cent, b->s.order, b->s.off, n, b->cb, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return KNNX_OK;
}
