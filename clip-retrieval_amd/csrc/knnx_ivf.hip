// knnx_ivf.hip -- IVF-Flat on the host side: the list layout, the single- and the multi-block scan, the device build
// (knnx_ivfb_*), the streaming build knnx_ivf_begin / add_assigned / end (see knnx_host.h) and the list-ordered ids of a built
// index (knnx_ivf_id_order / knnx_ivf_map_ids).

#include "knnx_host.h"
#include "knnx_id_order.h"

// IVF: the work list (ix->ivf1.work / ivf_nwork) of <= KNN_NQ queries already in HBM
int ivf_build_worklist(knnx_index* ix, const float* q_dev, int nq, hipStream_t st, const unsigned* gate) {
  {
    // coarse quantiser: top-nprobe centroids per query (the same flat scan over the [nlist, d] centroid rows), then
    // the work list = tiles of every list probed by at least one of the <= 32 queries, each with its query mask
    const int np = std::min(ix->ivf_nprobe, ix->ivf_nlist);
    if (np <= KNNX_MAX_K_FAST) {
      int r = scan_topk(ix->cent, q_dev, nq, np, ix->ivf1.Dc, ix->ivf1.Ic, st);
      if (r) return r;
      HIPCHK(launch_ivf_worklist(ix->ivf1.Ic, nq, np, ix->ivf_nlist, ix->ivf1.masks, ix->ivf.tile0, ix->ivf.ntile, ix->ivf.size,
                                 ix->ivf1.off, ix->ivf1.work, ix->ivf1.nwork, st));
    } else {
      // nprobe > 64 (BASELINE config 5 asks for 256): the centroid scan dumps every score, a selection kernel marks the
      // nprobe best lists of each query
      knnx_index* c = ix->cent;
      if (!ix->ivf1.scores) HIPCHK(ix->ivf1.scores.alloc((size_t)KNN_NQ * ix->ivf_nlist));
      HIPCHK(launch_prep(q_dev, nq, c->d, c->flat.qfrag, c->flat.thr_g, nullptr, 0, gate, st));
      ScanArgs ca{};
      ca.gate = gate;
      ca.X = c->rows;
      ca.N = c->ntotal;
      ca.d = c->d;
      ca.qfrag = c->flat.qfrag;
      ca.nq = nq;
      ca.k = 1;
      ca.cap = 2;
      ca.grid = c->n_cu;
      ca.mode = 2;
      ca.thr_g = c->flat.thr_g;
      ca.range_cap = (unsigned)ix->ivf_nlist;
      ca.range_s = ix->ivf1.scores;
      HIPCHK(launch_scan(ca, st));
      HIPCHK(launch_ivf_worklist_from_scores(ix->ivf1.scores, nq, np, ix->ivf_nlist, ix->ivf1.masks, ix->ivf.tile0, ix->ivf.ntile,
                                             ix->ivf.size, ix->ivf1.off, ix->ivf1.work, ix->ivf1.nwork, st));
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// IVF, more than 32 queries: the multi-block pass.  The 32-query scan keeps one block's hi / lo fragments in the LDS (d * 128 B:
// 128 KiB at d = 1024), so a batch of B queries used to be ceil(B / 32) passes, each with its own coarse scan, work-list kernels,
// list scan and merge (~0.55 ms of small kernels and launch gaps per pass on config 5's shard: 4.4 of the 7.2 ms of a 256-query
// batch at nprobe 16).  Here the blocks run SIDE BY SIDE: one prep, one coarse scan, one work-list build, one list scan, one merge
// for up to IVFM_BLK x 32 queries; workgroup g of a scan serves block g % nblk (knn_kernels.hip: knn_scan_kernel, nblk).  A list
// probed by queries of one block is read once (as before); probed from two blocks it is read by both (the L2 / MALL may catch the
// second read: the blocks walk their lists at the same time).  Results are those of the 32-query path, bit for bit: every block
// runs the same exact hi / lo scan over the same candidate set (reference call: clip_back.py:357-369, nprobe on the IVF branch).
// ---------------------------------------------------------------------------------------------
bool ivfm_usable(const knnx_index* ix, int nq, int k) {
  // (any batch size since the coarse quantiser of this pass is the score dump + radix select: at 32 queries and fewer it is one block)
  // (n_cu >= IVFM_BLK: every block needs a workgroup of its own, and the partial-list arrays hold n_cu slots -- KNNX_GRID can set fewer)
  return ix->ivf_nlist && ix->ivfm_ok && ix->cent && nq >= 1 && k <= KNNX_MAX_K_FAST && scan_cap(ix->d, k) > 0 && ix->n_cu >= IVFM_BLK;
}

// 0: buffers are there; 1: not available (the caller falls back to the 32-query passes; ivfm_ok is cleared)
int ivfm_alloc(knnx_index* ix) {
  if (ix->ivfm.alloc(ix->d, (size_t)ix->ivf_nlist, ix->capacity) == hipSuccess) return 0;
  (void)hipGetLastError();
  ix->ivfm_ok = 0;
  return 1;
}

// the coarse half of a multi-block pass (IVF-Flat below, IVF-SQ8 in knnx_ivfsq.hip): fragments of nq queries in nblk blocks (thr_c and,
// when given, thr_f reset), the centroid scores, the nprobe best lists of every query, the blocks' work lists in ix->ivfm
int ivfm_coarse_worklists(knnx_index* ix, const float* q_dev, int nq, int nblk, int grid, int* thr_f_or_null, hipStream_t st) {
  knnx_index* c = ix->cent;
  const int np = std::min(ix->ivf_nprobe, ix->ivf_nlist);
  HIPCHK(launch_prep_blocks(q_dev, nq, ix->d, ix->ivfm.qfrag, ix->ivfm.thr_c, thr_f_or_null, st));
  // coarse quantiser: ONE scan over the centroid rows dumps every block's scores (mode 2: no queues -- a top-nprobe queue scan of
  // 65 536 centroids spends its time pruning cold queues: 245 us for two blocks, profiles/r06k_*), a radix select marks the nprobe
  // best lists of every query (knn_kernels.hip: ivf_select_mark_kernel), whatever nprobe is
  ScanArgs ca{};
  ca.X = c->rows;
  ca.N = c->ntotal;
  ca.d = c->d;
  ca.qfrag = ix->ivfm.qfrag;
  ca.nq = nq;
  ca.grid = grid;
  ca.thr_g = ix->ivfm.thr_c;
  ca.nblk = nblk;
  ca.k = 1;
  ca.cap = 2;
  ca.mode = 2;
  ca.range_cap = (unsigned)ix->ivf_nlist;
  ca.range_s = ix->ivfm.scores;
  HIPCHK(launch_scan(ca, st));
  HIPCHK(launch_ivf_worklist_from_scores(ix->ivfm.scores, nq, np, ix->ivf_nlist, ix->ivfm.masks, ix->ivf.tile0, ix->ivf.ntile,
                                         ix->ivf.size, ix->ivfm.off, ix->ivfm.work, ix->ivfm.nwork, st, ix->ivfm.stride));
  if (ix->prof.on)  // tiles of the union of the blocks' lists (what one pass over shared lists would read): knnx_ivf_last_scan_tiles
    HIPCHK(launch_ivf_union_tiles(ix->ivfm.masks, nblk, ix->ivf_nlist, ix->ivf.ntile, ix->ivfm.nwork + IVFM_BLK, st));
  return 0;
}

// one pass of 1 .. 32 IVFM_BLK queries already in HBM
int scan_topk_ivf_multi(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st) {
  const int cap = scan_cap(ix->d, k);
  const int nblk = (nq + KNN_NQ - 1) / KNN_NQ;
  const int grid = std::max(1, ix->n_cu / nblk) * nblk;  // (part_* hold n_cu x 64 lists: grid <= n_cu whenever n_cu >= nblk)
  if (cap < 0 || nblk > IVFM_BLK || grid > std::max(ix->n_cu, nblk)) return fail(KNNX_E_STATE, "internal: multi-block IVF pass misuse");
  int r = ivfm_coarse_worklists(ix, q_dev, nq, nblk, grid, ix->ivfm.thr_f, st);
  if (r) return r;
  ScanArgs a{};
  a.X = ix->rows;
  a.N = ix->capacity;
  a.d = ix->d;
  a.qfrag = ix->ivfm.qfrag;
  a.nq = nq;
  a.k = k;
  a.cap = cap;
  a.grid = grid;
  a.mode = 0;
  a.thr_g = ix->ivfm.thr_f;
  a.part_s = ix->flat.part_s;
  a.part_i = ix->flat.part_i;
  a.part_n = ix->flat.part_n;
  a.work = ix->ivfm.work;
  a.nwork = ix->ivfm.nwork;
  a.nblk = nblk;
  a.work_stride = ix->ivfm.stride;
  HIPCHK(ix->prof.begin(ix->prof.on, st));
  HIPCHK(launch_scan(a, st));
  HIPCHK(ix->prof.end(ix->prof.on, st));
  HIPCHK(launch_merge_u32(ix->flat.part_s, ix->flat.part_i, ix->flat.part_n, grid - nblk + 1, KNN_NQ, k, nq, k, ix->id_base, ix->ivf.idmap, D_out, I_out,
                          nullptr, st, KNN_NQ, ix->ivfm.nwork, nblk, grid));
  ix->ivfm_last_blk = nblk;
  ix->ivfm_union_valid = ix->prof.on;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// IVF-Flat
// ---------------------------------------------------------------------------------------------
// the tile layout of the lists: list l holds rows [tile0[l] * 32, tile0[l] * 32 + size[l]) of the padded arena
struct TileLayout {
  std::vector<int64_t> src0;  // first row of every list in list-by-list order
  std::vector<unsigned> tile0, ntile, size;
  int64_t rows = 0, tiles = 0, prow = 0;  // rows the lists hold; tiles and rows of the padded arena
};
static int ivf_tile_layout(int nlist, const int64_t* list_sizes, TileLayout& t) {
  t.src0.resize(nlist), t.tile0.resize(nlist), t.ntile.resize(nlist), t.size.resize(nlist);
  for (int l = 0; l < nlist; ++l) {
    if (list_sizes[l] < 0) return fail(KNNX_E_ARG, "negative list size");
    t.src0[l] = t.rows;
    t.size[l] = (unsigned)list_sizes[l];
    t.ntile[l] = (unsigned)((list_sizes[l] + 31) / 32);
    t.tile0[l] = (unsigned)t.tiles;
    t.rows += list_sizes[l];
    t.tiles += t.ntile[l];
  }
  if (t.tiles * 32 > (int64_t)0xffffffffll) return fail(KNNX_E_UNSUPPORTED, "more than 2^32 padded rows per device");
  t.prow = std::max<int64_t>(t.tiles * 32, 32);
  return 0;
}
// the layout group and the single-block scratch of an index with these lists, the layout uploaded on the index's stream (the
// caller synchronises it before `t` goes away).  Both groups are empty when this fails.
static int ivf_layout_alloc(knnx_index* ix, const TileLayout& t) {
  const size_t nlist = t.size.size();
  IvfLayout& L = ix->ivf;
  IvfScratch& S = ix->ivf1;
  hipError_t e = hipSuccess;
  dev_alloc(e, L.tile0, nlist);
  dev_alloc(e, L.ntile, nlist);
  dev_alloc(e, L.size, nlist);
  dev_alloc(e, S.masks, nlist);
  dev_alloc(e, S.off, nlist);
  dev_alloc(e, S.nwork, 1);
  dev_alloc(e, S.work, (size_t)std::max<int64_t>(t.tiles, 1));
  dev_alloc(e, L.idmap, (size_t)t.prow);
  dev_alloc(e, L.inv, (size_t)std::max<int64_t>(t.rows, 1));
  dev_alloc(e, S.Ic, (size_t)KNN_NQ * KNNX_MAX_K_FAST);
  dev_alloc(e, S.Dc, (size_t)KNN_NQ * KNNX_MAX_K_FAST);
  if (e == hipSuccess) e = hipMemcpyAsync(L.tile0, t.tile0.data(), nlist * sizeof(unsigned), hipMemcpyHostToDevice, ix->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(L.ntile, t.ntile.data(), nlist * sizeof(unsigned), hipMemcpyHostToDevice, ix->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(L.size, t.size.data(), nlist * sizeof(unsigned), hipMemcpyHostToDevice, ix->stream);
  if (e == hipSuccess) return 0;
  (void)hipStreamSynchronize(ix->stream);
  ix->ivf = IvfLayout();
  ix->ivf1 = IvfScratch();
  return fail(e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP, std::string("IVF layout: ") + hipGetErrorString(e));
}

extern "C" int knnx_ivf_set_lists(knnx_index* ix, int nlist, const uint16_t* centroids_f16, const int64_t* list_sizes,
                                  const int64_t* ids) {
  if (!ix || nlist <= 0 || !centroids_f16 || !list_sizes || !ids) return fail(KNNX_E_ARG, "bad ivf_set_lists arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (ix->rows.borrowed) return fail(KNNX_E_STATE, "IVF needs an index that owns its rows");
  if (ix->pq.m) return fail(KNNX_E_STATE, "an IVF-PQ index is built through knnx_ivf_begin / knnx_ivf_add_assigned / knnx_ivf_end");
  if (ix->sq.on) return fail(KNNX_E_STATE, "an IVF-SQ8 index is built through knnx_ivf_begin / knnx_ivf_add_assigned / knnx_ivf_end");
  if (ix->ivf_nlist) return fail(KNNX_E_STATE, "lists are already set");
  TileLayout t;
  int r = ivf_tile_layout(nlist, list_sizes, t);
  if (r) return r;
  const int64_t run = t.rows;
  if (run != ix->ntotal) return fail(KNNX_E_ARG, "list sizes do not add up to ntotal (add the rows list by list first)");
  for (int64_t i = 0; i < run; ++i)
    if (ids[i] < ix->id_base || ids[i] - ix->id_base >= run) return fail(KNNX_E_ARG, "ids must be a permutation of [id_base, id_base + ntotal)");
  DevBuf<_Float16> dst;
  DevBuf<int64_t> ids_dev, src0_dev;
  if ((r = ivf_layout_alloc(ix, t))) return r;
  hipError_t e = dst.alloc((size_t)t.prow * ix->d);
  dev_alloc(e, ids_dev, (size_t)std::max<int64_t>(run, 1));
  dev_alloc(e, src0_dev, nlist);
  if (e == hipSuccess) e = hipMemcpy(ids_dev, ids, (size_t)run * sizeof(int64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(src0_dev, t.src0.data(), nlist * sizeof(int64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = launch_ivf_relayout(ix->rows, dst, ix->d, nlist, src0_dev, ix->ivf.tile0, ix->ivf.ntile, ix->ivf.size, ids_dev,
                            ix->id_base, run, ix->ivf.idmap, ix->ivf.inv, ix->stream);
  const hipError_t es = hipStreamSynchronize(ix->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    ix->ivf = IvfLayout();
    ix->ivf1 = IvfScratch();
    return fail(e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP, std::string("ivf_set_lists: ") + hipGetErrorString(e));
  }
  ix->rows = std::move(dst);
  ix->capacity = t.prow;
  ix->i8.release();  // (an IVF index does not use the int8 first stage: give a copy built while the index was flat back)
  r = knnx_create(ix->device, ix->d, KNNX_METRIC_INNER_PRODUCT, &ix->cent);
  if (r) return r;
  r = knnx_add_f16(ix->cent, centroids_f16, nlist);
  if (r) return r;
  ix->ivf_nlist = nlist;
  ix->ivf_nprobe = std::min(ix->ivf_nprobe, nlist);
  return KNNX_OK;
}

// ---------------------------------------------------------------------------------------------
// IVF-Flat build on the device (stands in for the autofaiss call of clip_index.py:12-66 for this index
// type).  Training: Lloyd iterations on a sample that stays resident in HBM -- assignment by knn_assign_kernel (MFMA-bound,
// every workgroup streams the whole centroid matrix), update by one workgroup per list over the host-sorted member order.
// Adding: two streaming passes over the embedding files, so that no second copy of a 256 GB shard is ever needed --
// pass 1 knnx_ivfb_assign (rows -> list ids, 4 bytes per row kept by the caller), pass 2 knnx_ivf_begin /
// knnx_ivf_add_assigned / knnx_ivf_end (rows scattered straight into the tile-padded list-sorted arena).  The host only
// does integer bookkeeping (bincount, prefix sums, stable ranks inside a chunk).
// ---------------------------------------------------------------------------------------------
struct knnx_ivf_builder {
  int device = 0, d = 0, nlist = 0;
  Stream stream;
  DevBuf<_Float16> cent;    // [nlist, d]
  DevBuf<_Float16> sample;  // resident training sample; borrowed after knnx_ivfb_set_sample_device
  int64_t n_sample = 0;
  DevBuf<_Float16> stage;   // one chunk of streamed rows
  DevBuf<int32_t> lists;    // assignment of a chunk / of the sample
  int64_t cap_rows = 0;
  DevBuf<int64_t> order, off;
  PinBuf pin;
  DevBuf<unsigned long long> hist;  // [nlist] list sizes accumulated by knnx_ivfb_assign_device
  std::vector<int32_t> h_lists;     // host scratch of knnx_ivfb_lloyd
  std::vector<int64_t> h_order, h_off;
};

extern "C" void knnx_ivfb_destroy(knnx_ivf_builder* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  delete b;
}

extern "C" int knnx_ivfb_create(int device, int d, int nlist, knnx_ivf_builder** out) {
  if (!out || nlist <= 0) return fail(KNNX_E_ARG, "bad ivfb_create arguments");
  *out = nullptr;
  if (d <= 0 || d % 256 != 0 || d > 1024) return fail(KNNX_E_UNSUPPORTED, "d must be a multiple of 256 and <= 1024");
  HIPCHK(hipSetDevice(device));
  knnx_ivf_builder* b = new knnx_ivf_builder();
  b->device = device;
  b->d = d;
  b->nlist = nlist;
  hipError_t e = b->stream.create();
  dev_alloc(e, b->cent, (size_t)nlist * d);
  dev_alloc(e, b->off, (size_t)nlist + 1);
  dev_alloc(e, b->hist, (size_t)nlist);
  if (e == hipSuccess) e = hipMemset(b->hist, 0, (size_t)nlist * sizeof(unsigned long long));
  if (e == hipSuccess) e = b->pin.ensure((size_t)IVFB_CHUNK * d * sizeof(_Float16));
  if (e != hipSuccess) {
    knnx_ivfb_destroy(b);
    return fail(e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP, std::string("ivfb_create: ") + hipGetErrorString(e));
  }
  *out = b;
  return KNNX_OK;
}

extern "C" int knnx_ivfb_set_centroids(knnx_ivf_builder* b, const uint16_t* centroids_f16) {
  if (!b || !centroids_f16) return fail(KNNX_E_ARG, "bad ivfb_set_centroids arguments");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpy(b->cent, centroids_f16, (size_t)b->nlist * b->d * sizeof(_Float16), hipMemcpyHostToDevice));
  return KNNX_OK;
}
extern "C" int knnx_ivfb_get_centroids(knnx_ivf_builder* b, uint16_t* centroids_f16) {
  if (!b || !centroids_f16) return fail(KNNX_E_ARG, "bad ivfb_get_centroids arguments");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(centroids_f16, b->cent, (size_t)b->nlist * b->d * sizeof(_Float16), hipMemcpyDeviceToHost));
  return KNNX_OK;
}

static int ivfb_rows_cap(knnx_ivf_builder* b, int64_t rows) {
  if (rows <= b->cap_rows) return 0;
  b->cap_rows = 0;
  b->lists.reset();
  HIPCHK(b->stage.alloc((size_t)std::min<int64_t>(rows, IVFB_CHUNK) * b->d));
  HIPCHK(b->lists.alloc((size_t)rows));
  b->cap_rows = rows;
  return 0;
}

// upload host rows in chunks through the pinned buffer into dst (device)
static int ivfb_upload(knnx_ivf_builder* b, const uint16_t* rows, int64_t n, _Float16* dst) {
  const size_t rb = (size_t)b->d * sizeof(_Float16);
  for (int64_t o = 0; o < n; o += IVFB_CHUNK) {
    const int64_t m = std::min(IVFB_CHUNK, n - o);
    memcpy(b->pin.p, rows + (size_t)o * b->d, (size_t)m * rb);
    HIPCHK(hipMemcpyAsync(dst + (size_t)o * b->d, b->pin.p, (size_t)m * rb, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  return 0;
}

extern "C" int knnx_ivfb_set_sample(knnx_ivf_builder* b, const uint16_t* rows_f16, int64_t n) {
  if (!b || !rows_f16 || n <= 0) return fail(KNNX_E_ARG, "bad ivfb_set_sample arguments");
  HIPCHK(hipSetDevice(b->device));
  b->order.reset();
  HIPCHK(b->sample.alloc((size_t)n * b->d));
  HIPCHK(b->order.alloc((size_t)n));
  b->n_sample = n;
  int r = ivfb_rows_cap(b, n);
  if (r) return r;
  return ivfb_upload(b, rows_f16, n, b->sample);
}

extern "C" int knnx_ivfb_assign_sample(knnx_ivf_builder* b, int32_t* lists_out) {
  if (!b || !lists_out || !b->sample) return fail(KNNX_E_ARG, "bad ivfb_assign_sample arguments (set a sample first)");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(launch_assign(b->cent, b->nlist, b->d, b->sample, b->n_sample, b->lists, b->stream));
  HIPCHK(hipMemcpyAsync(lists_out, b->lists, (size_t)b->n_sample * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return KNNX_OK;
}

extern "C" int knnx_ivfb_update(knnx_ivf_builder* b, const int64_t* order, const int64_t* off) {
  if (!b || !order || !off || !b->sample) return fail(KNNX_E_ARG, "bad ivfb_update arguments (set a sample first)");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(b->order, order, (size_t)b->n_sample * sizeof(int64_t), hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->off, off, (size_t)(b->nlist + 1) * sizeof(int64_t), hipMemcpyHostToDevice, b->stream));
  HIPCHK(launch_kmeans_update(b->sample, b->d, b->order, b->off, b->nlist, b->cent, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return KNNX_OK;
}

extern "C" int knnx_ivfb_assign(knnx_ivf_builder* b, const uint16_t* rows_f16, int64_t n, int32_t* lists_out) {
  if (!b || (n > 0 && (!rows_f16 || !lists_out)) || n < 0) return fail(KNNX_E_ARG, "bad ivfb_assign arguments");
  if (n == 0) return KNNX_OK;
  HIPCHK(hipSetDevice(b->device));
  int r = ivfb_rows_cap(b, std::min<int64_t>(n, IVFB_CHUNK));
  if (r) return r;
  const size_t rb = (size_t)b->d * sizeof(_Float16);
  for (int64_t o = 0; o < n; o += IVFB_CHUNK) {
    const int64_t m = std::min(IVFB_CHUNK, n - o);
    memcpy(b->pin.p, rows_f16 + (size_t)o * b->d, (size_t)m * rb);
    HIPCHK(hipMemcpyAsync(b->stage, b->pin.p, (size_t)m * rb, hipMemcpyHostToDevice, b->stream));
    HIPCHK(launch_assign(b->cent, b->nlist, b->d, b->stage, m, b->lists, b->stream));
    HIPCHK(hipMemcpyAsync(lists_out + o, b->lists, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  return KNNX_OK;
}


// ---- the same builder for rows that are already in HBM (SURVEY 8 row f1 at BASELINE config 5's size: a 256 GB shard cannot
// take a detour through host memory, and nothing of it needs to: the embeddings are produced on this GPU) ----------------
extern "C" int knnx_ivfb_set_sample_device(knnx_ivf_builder* b, const void* rows_dev, int64_t n) {
  if (!b || !rows_dev || n <= 0) return fail(KNNX_E_ARG, "bad ivfb_set_sample_device arguments");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  b->sample.borrow(rows_dev);  // the caller keeps it alive until the training is over
  HIPCHK(b->order.alloc((size_t)n));
  b->n_sample = n;
  return ivfb_rows_cap(b, n);
}

// centroid list_ids[i] := sample row sample_rows[i] (initial seeding, re-seeding of empty lists); host index arrays
extern "C" int knnx_ivfb_seed_from_sample(knnx_ivf_builder* b, const int32_t* list_ids, const int64_t* sample_rows, int64_t n) {
  if (!b || (n > 0 && (!list_ids || !sample_rows)) || n < 0 || !b->sample) return fail(KNNX_E_ARG, "bad ivfb_seed_from_sample arguments (set a sample first)");
  if (n == 0) return KNNX_OK;
  for (int64_t i = 0; i < n; ++i)
    if (list_ids[i] < 0 || list_ids[i] >= b->nlist || sample_rows[i] < 0 || sample_rows[i] >= b->n_sample)
      return fail(KNNX_E_ARG, "list id / sample row out of range");
  HIPCHK(hipSetDevice(b->device));
  DevBuf<int32_t> l_dev;
  DevBuf<int64_t> r_dev;
  HIPCHK(l_dev.alloc((size_t)n));
  hipError_t e = r_dev.alloc((size_t)n);
  if (e == hipSuccess) e = hipMemcpyAsync(l_dev, list_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(r_dev, sample_rows, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = launch_copy_rows(b->sample, b->d, r_dev, l_dev, n, b->cent, b->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
  if (e != hipSuccess) return fail(KNNX_E_HIP, std::string("ivfb_seed_from_sample: ") + hipGetErrorString(e));
  return KNNX_OK;
}

// One Lloyd iteration over the resident sample, driven from here: assignment kernel -> list ids to the host -> counting sort
// (member order = ascending sample row inside a list: the fixed summation order of knnx_ivfb_update) -> update kernel.
// sizes_out [nlist] (host, may be null): members per list, so that the caller can re-seed the empty ones.
extern "C" int knnx_ivfb_lloyd(knnx_ivf_builder* b, int64_t* sizes_out) {
  if (!b || !b->sample) return fail(KNNX_E_ARG, "bad ivfb_lloyd arguments (set a sample first)");
  HIPCHK(hipSetDevice(b->device));
  const int64_t n = b->n_sample;
  b->h_lists.resize((size_t)n);
  b->h_order.resize((size_t)n);
  b->h_off.assign((size_t)b->nlist + 1, 0);
  HIPCHK(launch_assign(b->cent, b->nlist, b->d, b->sample, n, b->lists, b->stream));
  HIPCHK(hipMemcpyAsync(b->h_lists.data(), b->lists, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  for (int64_t i = 0; i < n; ++i) b->h_off[(size_t)b->h_lists[i] + 1]++;
  if (sizes_out) for (int l = 0; l < b->nlist; ++l) sizes_out[l] = b->h_off[(size_t)l + 1];
  for (int l = 0; l < b->nlist; ++l) b->h_off[(size_t)l + 1] += b->h_off[l];
  {
    std::vector<int64_t> cur(b->h_off.begin(), b->h_off.end() - 1);
    for (int64_t i = 0; i < n; ++i) b->h_order[(size_t)cur[b->h_lists[i]]++] = i;
  }
  HIPCHK(hipMemcpyAsync(b->order, b->h_order.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->off, b->h_off.data(), (size_t)(b->nlist + 1) * sizeof(int64_t), hipMemcpyHostToDevice, b->stream));
  HIPCHK(launch_kmeans_update(b->sample, b->d, b->order, b->off, b->nlist, b->cent, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return KNNX_OK;
}

// pass 1 over device-resident rows: lists_dev[i] = list of row i (device int32 [n]); the list sizes accumulate in the builder
extern "C" int knnx_ivfb_assign_device(knnx_ivf_builder* b, const void* rows_dev, int64_t n, int32_t* lists_dev) {
  if (!b || (n > 0 && (!rows_dev || !lists_dev)) || n < 0) return fail(KNNX_E_ARG, "bad ivfb_assign_device arguments");
  if (n == 0) return KNNX_OK;
  HIPCHK(hipSetDevice(b->device));
  const int64_t step = (int64_t)1 << 22;  // rows per launch (grid size)
  for (int64_t o = 0; o < n; o += step) {
    const int64_t m = std::min(step, n - o);
    HIPCHK(launch_assign(b->cent, b->nlist, b->d, (const _Float16*)rows_dev + (size_t)o * b->d, m, lists_dev + o, b->stream));
  }
  HIPCHK(launch_ivf_hist(lists_dev, n, b->nlist, b->hist, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return KNNX_OK;
}

// list sizes seen by knnx_ivfb_assign_device so far -> sizes_out [nlist] (host); reset != 0 clears the counters afterwards
extern "C" int knnx_ivfb_list_sizes(knnx_ivf_builder* b, int64_t* sizes_out, int reset) {
  if (!b || !sizes_out) return fail(KNNX_E_ARG, "bad ivfb_list_sizes arguments");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "");
  HIPCHK(hipMemcpy(sizes_out, b->hist, (size_t)b->nlist * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (reset) HIPCHK(hipMemset(b->hist, 0, (size_t)b->nlist * sizeof(unsigned long long)));
  return KNNX_OK;
}

extern "C" int knnx_ivf_begin(knnx_index* ix, int nlist, const uint16_t* centroids_f16, const int64_t* list_sizes) {
  if (!ix || nlist <= 0 || !centroids_f16 || !list_sizes) return fail(KNNX_E_ARG, "bad ivf_begin arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (ix->rows.borrowed || ix->ntotal != 0 || ix->ivf_nlist || ix->ivfb.nlist) return fail(KNNX_E_STATE, "ivf_begin needs an empty index that owns its rows");
  // the centroids, and with them the encoder, live in the quantiser space: dq = d unless the index was given a d_out
  const int dq = ix->pq.m ? pq_dq(ix) : ix->d;
  if (dq != ix->d && !ix->pq.rot)
    return fail(KNNX_E_STATE, "an index with d_out = " + std::to_string(dq) + " != d = " + std::to_string(ix->d) +
                                  " needs its rotation [d_out][d] before knnx_ivf_begin (knnx_ivfpq_set_rotation): nothing else leads "
                                  "from the rows to the quantiser space");
  TileLayout t;
  int r = ivf_tile_layout(nlist, list_sizes, t);
  if (r) return r;
  ix->rows.reset();
  ix->capacity = 0;
  if ((r = ivf_layout_alloc(ix, t))) return r;
  const int64_t prow = t.prow;
  IvfBuild& B = ix->ivfb;
  hipError_t e = hipSuccess;
  if (ix->pq.m) {  // IVF-PQ: M code bytes per arena row, and the centroids on the device for the encoder
    dev_alloc(e, ix->pq.codes, (size_t)prow * ix->pq.m);
    if (e == hipSuccess) e = hipMemsetAsync(ix->pq.codes, 0, (size_t)prow * ix->pq.m, ix->stream);
    dev_alloc(e, ix->pq.bcent, (size_t)nlist * dq);
    if (e == hipSuccess) e = hipMemcpyAsync(ix->pq.bcent, centroids_f16, (size_t)nlist * dq * sizeof(_Float16), hipMemcpyHostToDevice, ix->stream);
    if (ix->pq.refine) {  // the row arena next to the code arena (pad rows are zero)
      if (e == hipSuccess) e = malloc_or_reclaim(ix, ix->rows, (size_t)prow * ix->d);
      if (e == hipSuccess) e = hipMemsetAsync(ix->rows, 0, (size_t)prow * ix->d * sizeof(_Float16), ix->stream);
    }
  } else if (ix->sq.on) {  // IVF-SQ8: d code bytes per arena row (pad rows are zero)
    dev_alloc(e, ix->sq.codes, (size_t)prow * ix->d);
    if (e == hipSuccess) e = hipMemsetAsync(ix->sq.codes, 0, (size_t)prow * ix->d, ix->stream);
  } else {
    dev_alloc(e, ix->rows, (size_t)prow * ix->d);
    if (e == hipSuccess) e = hipMemsetAsync(ix->rows, 0, (size_t)prow * ix->d * sizeof(_Float16), ix->stream);  // pad rows are zero
  }
  if (e == hipSuccess) e = hipMemsetAsync(ix->ivf.idmap, 0xFF, (size_t)prow * sizeof(int64_t), ix->stream);  // -1 on pad rows
  dev_alloc(e, B.rows, (size_t)IVFB_CHUNK * ix->d);
  if (ix->pq.rot) dev_alloc(e, B.rot, (size_t)IVFB_CHUNK * dq);
  dev_alloc(e, B.ids, (size_t)IVFB_CHUNK);
  dev_alloc(e, B.lists, (size_t)IVFB_CHUNK);
  dev_alloc(e, B.pos, (size_t)IVFB_CHUNK);
  const hipError_t es = hipStreamSynchronize(ix->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {  // nothing of a build that did not begin stays behind
    ix->ivf = IvfLayout();
    ix->ivf1 = IvfScratch();
    ix->ivfb = IvfBuild();
    ix->rows.reset();
    ix->pq.codes.reset();
    ix->pq.bcent.reset();
    ix->sq.codes.reset();
    return fail(e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP, std::string("ivf_begin: ") + hipGetErrorString(e));
  }
  ix->capacity = prow;
  ix->ivfb.cent.assign(centroids_f16, centroids_f16 + (size_t)nlist * dq);
  ix->ivfb.size.assign(t.size.begin(), t.size.end());
  ix->ivfb.tile0.assign(t.tile0.begin(), t.tile0.end());
  ix->ivfb.fill.assign(nlist, 0u);
  ix->ivfb.taken.assign((size_t)(prow + 63) / 64, 0ull);
  ix->ivfb.nlist = nlist;
  ix->ivfb.total = t.rows;
  ix->ivfb.added = 0;
  return KNNX_OK;
}

// claim arena slot (list, pos) for one row; caller holds ix->mu.  Returns false (message set) on a bad or reused slot.
static bool ivfb_claim(knnx_index* ix, int32_t list, int64_t pos) {
  if (list < 0 || list >= ix->ivfb.nlist) { fail(KNNX_E_ARG, "list id out of range"); return false; }
  if (pos < 0 || pos >= (int64_t)ix->ivfb.size[list]) { fail(KNNX_E_ARG, "position is not inside its list (0 <= pos < list size)"); return false; }
  const size_t slot = (size_t)ix->ivfb.tile0[list] * 32 + (size_t)pos;
  uint64_t& word = ix->ivfb.taken[slot >> 6];
  const uint64_t bit = 1ull << (slot & 63);
  if (word & bit) { fail(KNNX_E_ARG, "two rows were given the same (list, position)"); return false; }
  word |= bit;
  ix->ivfb.fill[list]++;
  return true;
}

// claim (lists[i], pos[i]) for all n rows of a call, or none of them: a refused call leaves the build as it was
static bool ivfb_claim_all(knnx_index* ix, const int32_t* lists, const int32_t* pos, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!ivfb_claim(ix, lists[i], pos[i])) {
      for (int64_t j = 0; j < i; ++j) {
        const size_t slot = (size_t)ix->ivfb.tile0[lists[j]] * 32 + (size_t)pos[j];
        ix->ivfb.taken[slot >> 6] &= ~(1ull << (slot & 63));
        ix->ivfb.fill[lists[j]]--;
      }
      return false;
    }
  return true;
}

// ---- codes in and out of a compressed index (knnx_ivfpq_add_codes / knnx_ivfsq_add_codes, ..._get_codes): `width` code bytes per row in
// `arena`.  The callers hold ix->mu and have checked their arguments and the state of their family.
// precomputed codes [n][width] (host) into an index between knnx_ivf_begin and knnx_ivf_end: the (list, position) rules of
// knnx_ivf_add_assigned, the scatter alone
int ivf_import_codes_locked(knnx_index* ix, uint8_t* arena, int width, const uint8_t* codes, int64_t n, const int64_t* ids, const int32_t* lists,
                            const int32_t* pos) {
  if (ix->ivfb.added + n > ix->ivfb.total) return fail(KNNX_E_ARG, "more rows than the list sizes announced");
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < ix->id_base || ids[i] - ix->id_base >= ix->ivfb.total) return fail(KNNX_E_ARG, "ids must lie in [id_base, id_base + total rows)");
  if (!ivfb_claim_all(ix, lists, pos, n)) return KNNX_E_ARG;
  // (ivfb.rows holds IVFB_CHUNK x d x 2 bytes: room for IVFB_CHUNK rows of `width` <= 2 d code bytes)
  for (int64_t o = 0; o < n; o += IVFB_CHUNK) {
    const int64_t m = std::min(IVFB_CHUNK, n - o);
    HIPCHK(hipMemcpy(ix->ivfb.rows, codes + (size_t)o * width, (size_t)m * width, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->ivfb.ids, ids + o, (size_t)m * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->ivfb.lists, lists + o, (size_t)m * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->ivfb.pos, pos + o, (size_t)m * 4, hipMemcpyHostToDevice));
    HIPCHK(launch_pq_scatter_codes((const uint8_t*)ix->ivfb.rows.p, m, width, ix->ivfb.lists, ix->ivfb.pos, ix->ivfb.ids, ix->ivf.tile0,
                                   ix->id_base, ix->ivfb.total, arena, ix->ivf.idmap, ix->ivf.inv, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
  }
  ix->ivfb.added += n;
  return KNNX_OK;
}

// every row of a built index in arena order: ids [ntotal], lists [ntotal], codes [ntotal][width].  tile0_h / size_h: the host copy of
// the layout.  A list's rows are contiguous in the arena: one copy per list, straight into place.
int ivf_export_codes_locked(knnx_index* ix, const uint8_t* arena, int width, const std::vector<unsigned>& tile0_h,
                            const std::vector<unsigned>& size_h, const char* family, int64_t* ids, int32_t* lists, uint8_t* codes) {
  if (set_dev(ix)) return KNNX_E_HIP;
  HIPCHK(hipStreamSynchronize(ix->stream));
  const size_t w = (size_t)width;
  std::vector<int64_t> idmap((size_t)ix->capacity);
  HIPCHK(hipMemcpy(idmap.data(), ix->ivf.idmap, idmap.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  int64_t o = 0;
  for (int l = 0; l < ix->ivf_nlist; ++l) {
    const size_t r0 = (size_t)tile0_h[l] * 32, n = size_h[l];
    if (n) HIPCHK(hipMemcpy(codes + (size_t)o * w, arena + r0 * w, n * w, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i, ++o) {
      ids[o] = idmap[r0 + i];
      lists[o] = l;
    }
  }
  return o == ix->ntotal ? KNNX_OK : fail(KNNX_E_STATE, std::string("internal: ") + family + " layout does not add up to ntotal");
}

extern "C" int knnx_ivf_add_assigned(knnx_index* ix, const uint16_t* rows_f16, int64_t n, const int64_t* ids, const int32_t* lists,
                                     const int32_t* pos) {
  if (!ix || (n > 0 && (!rows_f16 || !ids || !lists || !pos)) || n < 0) return fail(KNNX_E_ARG, "bad ivf_add_assigned arguments");
  if (n == 0) return KNNX_OK;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (!ix->ivfb.nlist) return fail(KNNX_E_STATE, "call knnx_ivf_begin first");
  if (ix->ivfb.added + n > ix->ivfb.total) return fail(KNNX_E_ARG, "more rows than the list sizes announced");
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < ix->id_base || ids[i] - ix->id_base >= ix->ivfb.total) return fail(KNNX_E_ARG, "ids must lie in [id_base, id_base + total rows)");
  if (!ivfb_claim_all(ix, lists, pos, n)) return KNNX_E_ARG;
  const size_t rb = (size_t)ix->d * sizeof(_Float16);
  int r = ensure_pin(ix, (size_t)IVFB_CHUNK * (rb + 16));
  if (r) return r;
  char* pin = (char*)ix->pin.p;
  for (int64_t o = 0; o < n; o += IVFB_CHUNK) {
    const int64_t m = std::min(IVFB_CHUNK, n - o);
    char* p_rows = pin;
    char* p_ids = p_rows + (size_t)IVFB_CHUNK * rb;
    char* p_lists = p_ids + (size_t)IVFB_CHUNK * 8;
    char* p_pos = p_lists + (size_t)IVFB_CHUNK * 4;
    memcpy(p_rows, rows_f16 + (size_t)o * ix->d, (size_t)m * rb);
    memcpy(p_ids, ids + o, (size_t)m * 8);
    memcpy(p_lists, lists + o, (size_t)m * 4);
    memcpy(p_pos, pos + o, (size_t)m * 4);
    HIPCHK(hipMemcpyAsync(ix->ivfb.rows, p_rows, (size_t)m * rb, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipMemcpyAsync(ix->ivfb.ids, p_ids, (size_t)m * 8, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipMemcpyAsync(ix->ivfb.lists, p_lists, (size_t)m * 4, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipMemcpyAsync(ix->ivfb.pos, p_pos, (size_t)m * 4, hipMemcpyHostToDevice, ix->stream));
    if (ix->pq.m) {  // IVF-PQ: the rows are encoded into their slots, not copied (OPQ: rotated first); a refine store also keeps them
      if (ix->pq.refine)
        HIPCHK(launch_ivf_scatter(ix->ivfb.rows, m, ix->d, ix->ivfb.lists, ix->ivfb.pos, ix->ivfb.ids, 0, ix->ivf.tile0, ix->id_base,
                                  ix->ivfb.total, ix->rows, ix->ivf.idmap, ix->ivf.inv, ix->stream));
      if (ix->pq.rot) HIPCHK(launch_rotate_f16(ix->pq.rot_w, ix->d, pq_dq(ix), ix->ivfb.rows, m, ix->ivfb.rot, ix->stream));
      HIPCHK(launch_pq_encode(ix->pq.rot ? ix->ivfb.rot.p : ix->ivfb.rows.p, m, pq_dq(ix), ix->pq.m, ix->ivfb.lists, ix->pq.bcent, ix->pq.cb,
                              ix->ivf.tile0, ix->ivfb.pos, ix->ivfb.ids, 0, ix->id_base, ix->ivfb.total,
                              ix->pq.codes, ix->ivf.idmap, ix->ivf.inv, ix->stream));
    } else if (ix->sq.on) {  // IVF-SQ8: the rows are encoded into their slots
      HIPCHK(launch_sq_encode(ix->ivfb.rows, m, ix->d, ix->ivfb.lists, ix->ivfb.pos, ix->ivfb.ids, 0, ix->ivf.tile0, ix->id_base,
                              ix->ivfb.total, ix->sq.vmin, ix->sq.scale, ix->sq.codes, ix->ivf.idmap, ix->ivf.inv, ix->stream));
    } else {
      HIPCHK(launch_ivf_scatter(ix->ivfb.rows, m, ix->d, ix->ivfb.lists, ix->ivfb.pos,
                                ix->ivfb.ids, 0, ix->ivf.tile0, ix->id_base, ix->ivfb.total, ix->rows, ix->ivf.idmap,
                                ix->ivf.inv, ix->stream));
      HIPCHK(launch_maxnorm(ix->ivfb.rows, m, ix->d, ix->flat.maxnorm, ix->stream));
    }
    HIPCHK(hipStreamSynchronize(ix->stream));
  }
  ix->ivfb.added += n;
  return KNNX_OK;
}

// The same pass for rows that are already in HBM (a shard generated or encoded on this GPU): row i carries id id0 + i and
// goes to the next free position of lists_dev[i] -- positions inside a list follow the order of the calls and of the rows
// inside a call, exactly what knn.build_ivf_index hands to knnx_ivf_add_assigned.  The list ids travel to the host once
// (4 bytes per row) for the position bookkeeping; the rows never leave the device.
extern "C" int knnx_ivf_add_assigned_device(knnx_index* ix, const void* rows_dev, int64_t n, int64_t id0, const int32_t* lists_dev) {
  if (!ix || (n > 0 && (!rows_dev || !lists_dev)) || n < 0) return fail(KNNX_E_ARG, "bad ivf_add_assigned_device arguments");
  if (n == 0) return KNNX_OK;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if (!ix->ivfb.nlist) return fail(KNNX_E_STATE, "call knnx_ivf_begin first");
  if (ix->ivfb.added + n > ix->ivfb.total) return fail(KNNX_E_ARG, "more rows than the list sizes announced");
  if (id0 < ix->id_base || id0 - ix->id_base + n > ix->ivfb.total) return fail(KNNX_E_ARG, "ids must lie in [id_base, id_base + total rows)");
  int r = ensure_pin(ix, (size_t)IVFB_CHUNK * 8);
  if (r) return r;
  int32_t* h_lists = (int32_t*)ix->pin.p;
  int32_t* h_pos = h_lists + IVFB_CHUNK;
  // Validate the WHOLE call before a single slot is claimed (a refusal half way through a call left claims behind
  // and the build could neither be retried nor finished): every list id in range, no list filled beyond its announced size.
  // Costs a second read-back of the 4-byte list ids (20 ms per 125 M rows).
  {
    std::vector<uint32_t> add((size_t)ix->ivfb.nlist, 0u);
    for (int64_t o = 0; o < n; o += IVFB_CHUNK) {
      const int64_t m = std::min(IVFB_CHUNK, n - o);
      HIPCHK(hipMemcpyAsync(h_lists, lists_dev + o, (size_t)m * 4, hipMemcpyDeviceToHost, ix->stream));
      HIPCHK(hipStreamSynchronize(ix->stream));
      for (int64_t i = 0; i < m; ++i) {
        const int32_t l = h_lists[i];
        if (l < 0 || l >= ix->ivfb.nlist) return fail(KNNX_E_ARG, "list id out of range (nothing was added)");
        if ((uint64_t)ix->ivfb.fill[l] + ++add[l] > (uint64_t)ix->ivfb.size[l])
          return fail(KNNX_E_ARG, "a list would receive more rows than its announced size (nothing was added)");
      }
    }
  }
  for (int64_t o = 0; o < n; o += IVFB_CHUNK) {
    const int64_t m = std::min(IVFB_CHUNK, n - o);
    HIPCHK(hipMemcpyAsync(h_lists, lists_dev + o, (size_t)m * 4, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    for (int64_t i = 0; i < m; ++i) {
      const int32_t l = h_lists[i];
      const int64_t p = ix->ivfb.fill[l];
      // cannot fail after the validation above unless host-variant calls claimed positions out of order in this list
      if (!ivfb_claim(ix, l, p)) return KNNX_E_ARG;
      h_pos[i] = (int32_t)p;
    }
    HIPCHK(hipMemcpyAsync(ix->ivfb.pos, h_pos, (size_t)m * 4, hipMemcpyHostToDevice, ix->stream));
    const _Float16* src = (const _Float16*)rows_dev + (size_t)o * ix->d;
    if (ix->pq.m) {
      if (ix->pq.refine)
        HIPCHK(launch_ivf_scatter(src, m, ix->d, lists_dev + o, ix->ivfb.pos, nullptr, id0 + o, ix->ivf.tile0, ix->id_base, ix->ivfb.total,
                                  ix->rows, ix->ivf.idmap, ix->ivf.inv, ix->stream));
      if (ix->pq.rot) HIPCHK(launch_rotate_f16(ix->pq.rot_w, ix->d, pq_dq(ix), src, m, ix->ivfb.rot, ix->stream));
      HIPCHK(launch_pq_encode(ix->pq.rot ? ix->ivfb.rot.p : src, m, pq_dq(ix), ix->pq.m, lists_dev + o, ix->pq.bcent, ix->pq.cb, ix->ivf.tile0, ix->ivfb.pos,
                              nullptr, id0 + o, ix->id_base, ix->ivfb.total, ix->pq.codes, ix->ivf.idmap, ix->ivf.inv, ix->stream));
    } else if (ix->sq.on) {
      HIPCHK(launch_sq_encode(src, m, ix->d, lists_dev + o, ix->ivfb.pos, nullptr, id0 + o, ix->ivf.tile0, ix->id_base, ix->ivfb.total,
                              ix->sq.vmin, ix->sq.scale, ix->sq.codes, ix->ivf.idmap, ix->ivf.inv, ix->stream));
    } else {
      HIPCHK(launch_ivf_scatter(src, m, ix->d, lists_dev + o, ix->ivfb.pos, nullptr, id0 + o, ix->ivf.tile0, ix->id_base,
                                ix->ivfb.total, ix->rows, ix->ivf.idmap, ix->ivf.inv, ix->stream));
      HIPCHK(launch_maxnorm(src, m, ix->d, ix->flat.maxnorm, ix->stream));
    }
    HIPCHK(hipStreamSynchronize(ix->stream));
  }
  ix->ivfb.added += n;
  return KNNX_OK;
}

extern "C" int knnx_ivf_end(knnx_index* ix) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  int nlist;
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    if (set_dev(ix)) return KNNX_E_HIP;
    if (!ix->ivfb.nlist) return fail(KNNX_E_STATE, "call knnx_ivf_begin first");
    if (ix->ivfb.added != ix->ivfb.total) return fail(KNNX_E_STATE, "fewer rows were added than the list sizes announced");
    nlist = ix->ivfb.nlist;
    for (int l = 0; l < nlist; ++l)
      if (ix->ivfb.fill[l] != ix->ivfb.size[l]) return fail(KNNX_E_STATE, "a list received fewer rows than its announced size");
    if (ix->pq.m) {
      ix->pq.tile0_h.assign(ix->ivfb.tile0.begin(), ix->ivfb.tile0.end());
      ix->pq.size_h.assign(ix->ivfb.size.begin(), ix->ivfb.size.end());
      ix->pq.slab_np = 0;  // (M = 256: the slab width is recomputed from these sizes)
      ix->pq.bcent.reset();
      ix->pq.rot_w.reset();
    }
    if (ix->sq.on) {
      ix->sq.tile0_h.assign(ix->ivfb.tile0.begin(), ix->ivfb.tile0.end());
      ix->sq.size_h.assign(ix->ivfb.size.begin(), ix->ivfb.size.end());
    }
    std::vector<uint32_t>().swap(ix->ivfb.size);
    std::vector<uint32_t>().swap(ix->ivfb.fill);
    std::vector<uint32_t>().swap(ix->ivfb.tile0);
    std::vector<uint64_t>().swap(ix->ivfb.taken);
    ix->ivfb.rows.reset(), ix->ivfb.rot.reset(), ix->ivfb.ids.reset(), ix->ivfb.lists.reset(), ix->ivfb.pos.reset();
  }
  // (the coarse quantiser is a flat index in the quantiser space; ix->pq is settled by now, so the width is read without the lock)
  int r = knnx_create(ix->device, ix->pq.m ? pq_dq(ix) : ix->d, KNNX_METRIC_INNER_PRODUCT, &ix->cent);
  if (r) return r;
  r = knnx_add_f16(ix->cent, ix->ivfb.cent.data(), nlist);
  if (r) return r;
  std::lock_guard<std::mutex> lk(ix->mu);
  ix->ntotal = ix->ivfb.total;
  ix->ivf_nlist = nlist;
  ix->ivf_nprobe = std::min(ix->ivf_nprobe, nlist);
  ix->ivfb = IvfBuild();
  return KNNX_OK;
}

extern "C" int knnx_ivf_set_nprobe(knnx_index* ix, int nprobe) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  if (nprobe < 1) return fail(KNNX_E_ARG, "nprobe must be >= 1");
  std::lock_guard<std::mutex> lk(ix->mu);
  ix->ivf_nprobe = nprobe;
  return KNNX_OK;
}

extern "C" int knnx_ivf_nlist(const knnx_index* ix) { return ix ? ix->ivf_nlist : 0; }
extern "C" int knnx_ivf_nprobe(const knnx_index* ix) { return ix ? ix->ivf_nprobe : 0; }

// IVF: 32-row tiles in the work list of the most recent scan (rows of the probed lists, padded to tiles): what that scan
// read from HBM is tiles * 32 * d * 2 bytes -- the measured side of "(nprobe / nlist) * N * d * 2" 
extern "C" int knnx_ivf_last_scan_tiles(knnx_index* ix, int64_t* tiles) {
  if (!ix || !tiles) return fail(KNNX_E_ARG, "bad ivf_last_scan_tiles arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->ivf_nlist) return fail(KNNX_E_STATE, "not an IVF index");
  if (set_dev(ix)) return KNNX_E_HIP;
  HIPCHK(hipStreamSynchronize(ix->stream));
  if (ix->ivfm_last_blk > 0) {  // the multi-block pass: every block walks its own list of tiles
    unsigned n[IVFM_BLK] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpy(n, ix->ivfm.nwork, (size_t)ix->ivfm_last_blk * sizeof(unsigned), hipMemcpyDeviceToHost));
    *tiles = 0;
    for (int b = 0; b < ix->ivfm_last_blk; ++b) *tiles += (int64_t)n[b];
    return KNNX_OK;
  }
  unsigned n = 0;
  HIPCHK(hipMemcpy(&n, ix->ivf1.nwork, sizeof(unsigned), hipMemcpyDeviceToHost));
  *tiles = (int64_t)n;
  return KNNX_OK;
}

// the same for the UNION of the lists the blocks of the most recent multi-block pass probed (a list counted once however many
// blocks read it): the bytes a single pass over shared lists would have read.  Needs profiling on (knnx_profile_enable) during the
// search; a single-block scan reports its own tiles.
extern "C" int knnx_ivf_last_scan_union_tiles(knnx_index* ix, int64_t* tiles) {
  if (!ix || !tiles) return fail(KNNX_E_ARG, "bad ivf_last_scan_union_tiles arguments");
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    if (!ix->ivf_nlist) return fail(KNNX_E_STATE, "not an IVF index");
    if (ix->ivfm_last_blk > 0) {
      if (!ix->ivfm_union_valid) return fail(KNNX_E_STATE, "the union of the lists is counted only while profiling is enabled (knnx_profile_enable)");
      if (set_dev(ix)) return KNNX_E_HIP;
      HIPCHK(hipStreamSynchronize(ix->stream));
      unsigned n = 0;
      HIPCHK(hipMemcpy(&n, ix->ivfm.nwork + IVFM_BLK, sizeof(unsigned), hipMemcpyDeviceToHost));
      *tiles = (int64_t)n;
      return KNNX_OK;
    }
  }
  return knnx_ivf_last_scan_tiles(ix, tiles);
}

// ---------------------------------------------------------------------------------------------
// List-ordered ids (include/knnx.h; the reference's reorder_metadata_by_ivf_index: ivf_metadata_ordering.py:46-64 builds the mapping
// with a Python loop over the lists and keeps ntotal x 8 bytes of it on the host, clip_back.py:350-369 applies it with np.take).
// Here the mapping is a function of the layout the index owns: ordinal = dense0[list] + position.  Neither entry point takes
// knnx_index::mu -- the layout is immutable once the index is built -- so a translation never waits for a scan; they serialise among
// themselves on IdOrder::mu and run on IdOrder::stream.  What they read without the lock (ivf_nlist, ivfb.nlist, ntotal, id_base) is
// settled by knnx_ivf_end / knnx_ivf_set_lists.
// ---------------------------------------------------------------------------------------------
static int ido_refuse(const knnx_index* ix, const char* who) {
  if (ix->ivfb.nlist)
    return fail(KNNX_E_STATE, std::string(who) + ": the index is between knnx_ivf_begin and knnx_ivf_end: its lists are not complete (call knnx_ivf_end first)");
  if (!ix->ivf_nlist) return fail(KNNX_E_STATE, std::string(who) + ": a flat index has no inverted lists to order its ids by");
  if (ix->ntotal <= 0) return fail(KNNX_E_STATE, std::string(who) + ": the index is empty");
  return 0;
}

// dense0 on the host and the device, the stream; caller holds ido.mu and has set the device.  Once per index.
static int ido_prepare(knnx_index* ix) {
  IdOrder& S = ix->ido;
  if (S.ready) return 0;
  if (!S.stream) HIPCHK(S.stream.create());
  const int nlist = ix->ivf_nlist;
  HIPCHK(hipStreamSynchronize(ix->stream));  // (this once: whatever laid the layout down has finished)
  std::vector<unsigned> size((size_t)nlist);
  HIPCHK(hipMemcpyAsync(size.data(), ix->ivf.size, (size_t)nlist * sizeof(unsigned), hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));
  ido_dense0(size.data(), nlist, S.dense0_h);
  if (S.dense0_h[(size_t)nlist] != ix->ntotal) return fail(KNNX_E_STATE, "internal: the list sizes do not add up to ntotal");
  HIPCHK(S.dense0.alloc((size_t)nlist + 1));
  hipError_t e = hipMemcpyAsync(S.dense0, S.dense0_h.data(), ((size_t)nlist + 1) * sizeof(int64_t), hipMemcpyHostToDevice, S.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(S.stream);
  if (e != hipSuccess) {
    S.dense0.reset();
    return fail(KNNX_E_HIP, std::string("id order: ") + hipGetErrorString(e));
  }
  S.ready = true;
  return 0;
}

extern "C" int knnx_ivf_id_order(knnx_index* ix, int64_t* old_to_new, int64_t* new_to_old) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  if (!old_to_new && !new_to_old) return fail(KNNX_E_ARG, "knnx_ivf_id_order: old_to_new and new_to_old are both null");
  int r = ido_refuse(ix, "knnx_ivf_id_order");
  if (r) return r;
  IdOrder& S = ix->ido;
  std::lock_guard<std::mutex> lk(S.mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if ((r = ido_prepare(ix))) return r;
  // consecutive ranges of ordinals (new_to_old) / ids (old_to_new) through ONE staging buffer of a chunk: nothing here is proportional
  // to ntotal on the device.  old_to_new comes from inv by the kernel of knnx_ivf_map_ids (thread per id), so both arrays leave the
  // device as contiguous slices and the host only copies.
  const IdoChunks plan(ix->ntotal, ido_chunk_from_env(getenv("KNNX_ID_ORDER_CHUNK")));
  DevBuf<int64_t> stage;
  PinBuf pin;
  HIPCHK(stage.alloc((size_t)plan.staging()));
  HIPCHK(pin.ensure((size_t)plan.staging() * sizeof(int64_t)));
  for (int64_t c = 0; c < plan.count(); ++c) {
    const int64_t o0 = plan.first(c), m = plan.len(c);
    if (new_to_old) {
      HIPCHK(launch_ivf_new_to_old(ix->ivf.idmap, ix->capacity, ix->ivf.tile0, S.dense0, ix->ivf_nlist, o0, m, stage, S.stream));
      HIPCHK(hipMemcpyAsync(pin.p, stage, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost, S.stream));
      HIPCHK(hipStreamSynchronize(S.stream));
      memcpy(new_to_old + o0, pin.p, (size_t)m * sizeof(int64_t));
    }
    if (old_to_new) {
      HIPCHK(launch_ivf_map_ids(ix->ivf.inv, ix->id_base, ix->ntotal, ix->ivf.tile0, S.dense0, ix->ivf_nlist, nullptr, o0, m, stage, S.stream));
      HIPCHK(hipMemcpyAsync(pin.p, stage, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost, S.stream));
      HIPCHK(hipStreamSynchronize(S.stream));
      memcpy(old_to_new + o0, pin.p, (size_t)m * sizeof(int64_t));
    }
  }
  return KNNX_OK;
}

extern "C" int knnx_ivf_map_ids(knnx_index* ix, const int64_t* ids, int64_t n, int64_t* out) {
  if (!ix) return fail(KNNX_E_ARG, "index is null");
  if (n < 0 || (n > 0 && (!ids || !out))) return fail(KNNX_E_ARG, "bad ivf_map_ids arguments");
  int r = ido_refuse(ix, "knnx_ivf_map_ids");
  if (r) return r;
  if (n == 0) return KNNX_OK;
  // the whole request is checked on the host before anything is launched: a refusal leaves `out` as it was
  const int64_t bad = ido_first_bad(ids, n, ix->id_base, ix->ntotal);
  if (bad >= 0)
    return fail(KNNX_E_ARG, "knnx_ivf_map_ids: id " + std::to_string(ids[bad]) + " at position " + std::to_string(bad) +
                                " is neither -1 nor in [" + std::to_string(ix->id_base) + ", " + std::to_string(ix->id_base + ix->ntotal) + ")");
  IdOrder& S = ix->ido;
  std::lock_guard<std::mutex> lk(S.mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  if ((r = ido_prepare(ix))) return r;
  const int64_t chunk = ido_chunk_from_env(getenv("KNNX_ID_ORDER_CHUNK"));
  if (S.cap < std::min(n, chunk)) {  // grow the staging: a power of two >= 1024 ids, one chunk at the most
    int64_t want = 1024;
    while (want < std::min(n, chunk)) want *= 2;
    want = std::min(want, chunk);
    S.cap = 0;
    HIPCHK(S.pin.ensure((size_t)want * sizeof(int64_t)));
    HIPCHK(S.dev.alloc((size_t)want));
    S.cap = want;
  }
  const int64_t step = std::min(S.cap, chunk);
  for (int64_t o = 0; o < n; o += step) {
    const int64_t m = std::min(step, n - o);
    memcpy(S.pin.p, ids + o, (size_t)m * sizeof(int64_t));
    HIPCHK(hipMemcpyAsync(S.dev, S.pin.p, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, S.stream));
    HIPCHK(launch_ivf_map_ids(ix->ivf.inv, ix->id_base, ix->ntotal, ix->ivf.tile0, S.dense0, ix->ivf_nlist, S.dev, 0, m, S.dev, S.stream));
    HIPCHK(hipMemcpyAsync(S.pin.p, S.dev, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    memcpy(out + o, S.pin.p, (size_t)m * sizeof(int64_t));
  }
  return KNNX_OK;
}
