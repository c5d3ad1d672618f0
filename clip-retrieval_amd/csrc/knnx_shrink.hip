// knnx_shrink.hip -- removing ids from a BUILT IVF index of any kind (IVF-Flat, IVF-PQ with its rotation / refine store / M = 256 /
// threshold scan, IVF-SQ8): knnx_ivf_remove_ids / knnx_ivf_remove_stats (include/knnx.h, "Shrinking a built index").  The
// arithmetic is knnx_shrink_plan.h, the kernels knn_shrink_kernels.hip.
//
// Like a call that grows the index (knnx_grow.hip) a removal is OUT OF PLACE and all or nothing: the survivors are renumbered, the new
// layout, id maps and arenas are allocated and filled next to the old ones, and only when all of that has succeeded does ivf_swap_in()
// make them the index, under knnx_index::mu and IdOrder::mu.  A search from another thread sees the index before or after the call; a
// failure leaves it exactly as it was.  A call that names no row of the index touches no device memory at all.

#include "knnx_host.h"
#include "knnx_shrink_plan.h"

namespace {

// the state a call builds next to the index
struct Shrunk {
  DevBuf<uint8_t> dead;        // [whole blocks of ids] 1: the id is removed
  DevBuf<uint32_t> rank;       // [whole blocks of ids] new id - id_base of every survivor
  DevBuf<uint32_t> blocksum;   // [blocks] survivors of a block, then its exclusive offset
  DevBuf<uint32_t> tmask, tpos;  // [old tiles] survivor mask; survivors of the list in front of the tile, then dst0
  DevBuf<unsigned> size_new;   // [nlist]
  DevBuf<int64_t> ids;         // one chunk of the caller's ids
  IvfLayout L;
  DevBuf<uint4> work;
  DevBuf<_Float16> rows;
  DevBuf<uint8_t> pq_codes, sq_codes;
  std::vector<unsigned> tile0, ntile, size;  // the new layout on the host
  int64_t tiles = 0, prow = 0, ntotal = 0;
  Event ev[5];                 // start | mark | plan | move | ids
  ShrinkStats stats;
};

int hip_fail(const char* who, hipError_t e) {
  (void)hipGetLastError();
  return fail(e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP, std::string(who) + ": " + hipGetErrorString(e) + " (nothing was removed)");
}

// an index that can shrink: built, IVF, owning its rows
int shrink_refuse(const knnx_index* ix, const char* who) {
  if (ix->ivfb.nlist)
    return fail(KNNX_E_ARG, std::string(who) + ": the index is between knnx_ivf_begin and knnx_ivf_end (finish the build first; nothing was removed)");
  if (!ix->ivf_nlist || !ix->cent) return fail(KNNX_E_ARG, std::string(who) + ": not a built IVF index (nothing was removed)");
  if (ix->rows.borrowed) return fail(KNNX_E_ARG, std::string(who) + ": the index borrows its rows (nothing was removed)");
  return 0;
}

int shrink_run(knnx_index* ix, const char* who, const int64_t* ids, int64_t n, Shrunk& G) {
  const int nlist = ix->ivf_nlist, d = ix->d;
  const int64_t N = ix->ntotal, id_lo = ix->id_base, prow_old = ix->capacity, tiles_old = prow_old / 32;
  const int64_t nblk = shrink_blocks(N);
  const size_t nl = (size_t)nlist;
  const bool has_rows = (!ix->pq.m && !ix->sq.on) || ix->pq.refine;
  hipStream_t st = ix->stream;
  int r;
  if ((r = scratch_acquire(ix, st))) return r;
  // ---- mark
  const int64_t cap = std::min<int64_t>(n, IVFB_CHUNK);
  hipError_t e = hipSuccess;
  dev_alloc(e, G.dead, (size_t)nblk * SHRINK_BLOCK);
  dev_alloc(e, G.rank, (size_t)nblk * SHRINK_BLOCK);
  dev_alloc(e, G.blocksum, (size_t)nblk);
  dev_alloc(e, G.tmask, (size_t)tiles_old);
  dev_alloc(e, G.tpos, (size_t)tiles_old);
  dev_alloc(e, G.size_new, nl);
  dev_alloc(e, G.ids, (size_t)cap);
  for (Event& ev : G.ev)
    if (e == hipSuccess) e = ev.create();
  if (e != hipSuccess) return hip_fail(who, e);
  if ((r = ensure_pin(ix, (size_t)cap * sizeof(int64_t)))) return r;
  HIPCHK(hipEventRecord(G.ev[0], st));
  HIPCHK(hipMemsetAsync(G.dead, 0, (size_t)nblk * SHRINK_BLOCK, st));
  for (int64_t o = 0; o < n; o += cap) {
    const int64_t m = std::min(cap, n - o);
    memcpy(ix->pin.p, ids + o, (size_t)m * sizeof(int64_t));
    HIPCHK(hipMemcpyAsync(G.ids, ix->pin.p, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(launch_ivf_shrink_mark(G.ids, m, id_lo, N, G.dead, st));
    HIPCHK(hipStreamSynchronize(st));  // (the pinned buffer is reused by the next chunk)
  }
  HIPCHK(hipEventRecord(G.ev[1], st));
  // ---- plan: the rank of every survivor ...
  std::vector<uint32_t> sums((size_t)nblk), off;
  HIPCHK(launch_ivf_shrink_rank_sum(G.dead, N, G.blocksum, st));
  HIPCHK(hipMemcpyAsync(sums.data(), G.blocksum, sums.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  // ... and, independent of it, the survivors of every tile and list
  HIPCHK(launch_ivf_shrink_mask(ix->ivf.idmap, prow_old, id_lo, N, G.dead, G.tmask, st));
  HIPCHK(launch_ivf_shrink_list_scan(ix->ivf.tile0, ix->ivf.ntile, nlist, G.tmask, G.tpos, G.size_new, st));
  std::vector<unsigned> size_old(nl), size_dev(nl);
  HIPCHK(hipMemcpyAsync(size_dev.data(), G.size_new, nl * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(size_old.data(), ix->ivf.size, nl * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  int64_t survivors = 0;
  int pr = shrink_block_scan(sums.data(), nblk, N, off, survivors);
  if (pr) return fail(KNNX_E_STATE, std::string(who) + ": internal: the survivor counts of the id scan are inconsistent (nothing was removed)");
  std::vector<int64_t> size_new(size_dev.begin(), size_dev.end());
  pr = shrink_layout(nlist, size_old.data(), size_new.data(), survivors, prow_old, G.tile0, G.ntile, G.size, G.tiles, G.prow);
  if (pr == SHRINK_E_ROWS) return fail(KNNX_E_STATE, std::string(who) + ": internal: more than 2^32 padded rows after a removal (nothing was removed)");
  if (pr == SHRINK_E_COUNT)
    return fail(KNNX_E_STATE, std::string(who) + ": internal: the new list sizes do not add up to the survivors of the id scan (nothing was removed)");
  if (pr) return fail(KNNX_E_STATE, std::string(who) + ": internal: a list would grow by a removal (nothing was removed)");
  G.ntotal = survivors;
  G.stats.n_removed = N - survivors;
  if (survivors == N) return 0;  // (cannot happen: the caller saw an id in range; nothing is swapped then)
  // ---- the new state
  const size_t prow = (size_t)G.prow;
  const int64_t row_bytes = (ix->pq.m ? (int64_t)ix->pq.m : 0) + (ix->sq.on ? (int64_t)d : 0) + (has_rows ? (int64_t)2 * d : 0);
  G.stats.moved_bytes = survivors * row_bytes;
  dev_alloc(e, G.L.tile0, nl);
  dev_alloc(e, G.L.ntile, nl);
  dev_alloc(e, G.L.size, nl);
  dev_alloc(e, G.L.idmap, prow);
  dev_alloc(e, G.L.inv, (size_t)std::max<int64_t>(survivors, 1));
  dev_alloc(e, G.work, (size_t)std::max<int64_t>(G.tiles, 1));
  if (ix->pq.m) dev_alloc(e, G.pq_codes, prow * (size_t)ix->pq.m);
  if (ix->sq.on) dev_alloc(e, G.sq_codes, prow * (size_t)d);
  if (has_rows) dev_alloc(e, G.rows, prow * (size_t)d);
  if (e == hipSuccess) e = hipMemcpyAsync(G.blocksum, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(G.L.tile0, G.tile0.data(), nl * sizeof(unsigned), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(G.L.ntile, G.ntile.data(), nl * sizeof(unsigned), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(G.L.size, G.size.data(), nl * sizeof(unsigned), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_ivf_shrink_rank_apply(G.dead, N, G.blocksum, G.rank, st);
  if (e == hipSuccess) e = launch_ivf_shrink_dst0(ix->ivf.tile0, ix->ivf.ntile, G.L.tile0, nlist, G.tpos, st);
  if (e == hipSuccess) e = hipEventRecord(G.ev[2], st);
  // ---- move, then the pad rows of every list (an index without a tile keeps one tile of zeros)
  struct Payload {
    const void* src;
    void* dst;
    int width;
  } pay[3] = {{ix->pq.codes.p, G.pq_codes.p, ix->pq.m}, {ix->sq.codes.p, G.sq_codes.p, d}, {ix->rows.p, G.rows.p, 2 * d}};
  for (const Payload& p : pay) {
    if (!p.dst || e != hipSuccess) continue;
    if (G.tiles == 0) {
      e = hipMemsetAsync(p.dst, 0, prow * (size_t)p.width, st);
      continue;
    }
    e = launch_ivf_shrink_move(p.src, p.dst, p.width, G.tmask, G.tpos, tiles_old, ix->n_cu, st);
    if (e == hipSuccess) e = launch_ivf_shrink_pads(p.dst, p.width, G.L.tile0, G.L.ntile, G.L.size, nlist, st);
  }
  if (e == hipSuccess) e = hipEventRecord(G.ev[3], st);
  // ---- ids
  if (e == hipSuccess) e = hipMemsetAsync(G.L.idmap, 0xFF, prow * sizeof(int64_t), st);
  if (e == hipSuccess) e = launch_ivf_shrink_ids(ix->ivf.idmap, prow_old, id_lo, N, G.tmask, G.tpos, G.rank, G.L.idmap, G.L.inv, st);
  if (e == hipSuccess) e = hipEventRecord(G.ev[4], st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    return hip_fail(who, e);
  }
  return 0;
}

}  // namespace

extern "C" int knnx_ivf_remove_ids(knnx_index* ix, const int64_t* ids, int64_t n, int64_t* n_removed) {
  const char* who = "knnx_ivf_remove_ids";
  if (!ix) return fail(KNNX_E_ARG, std::string(who) + ": index is null");
  if (n < 0 || (n > 0 && !ids)) return fail(KNNX_E_ARG, std::string(who) + ": bad arguments (nothing was removed)");
  std::lock_guard<std::mutex> lk(ix->mu);
  int r = shrink_refuse(ix, who);
  if (r) return r;
  // an id that names a row?  (checked on the host: a call without one touches no device memory and leaves every cache as it was)
  bool any = false;
  for (int64_t i = 0; i < n && !any; ++i) any = shrink_index(ids[i], ix->id_base, ix->ntotal) < (uint64_t)ix->ntotal;
  ShrinkStats none;
  none.calls = ix->shrink.calls + 1;
  if (!any) {
    ix->shrink = none;
    if (n_removed) *n_removed = 0;
    return KNNX_OK;
  }
  if (set_dev(ix)) return KNNX_E_HIP;
  Shrunk G;
  if ((r = shrink_run(ix, who, ids, n, G))) return r;
  if (G.ntotal == ix->ntotal) return fail(KNNX_E_STATE, std::string(who) + ": internal: an id in range marked no row (nothing was removed)");
  float ms[4] = {0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) HIPCHK(hipEventElapsedTime(&ms[i], G.ev[i], G.ev[i + 1]));
  G.stats.mark_ms = ms[0], G.stats.plan_ms = ms[1], G.stats.move_ms = ms[2], G.stats.ids_ms = ms[3];
  G.stats.calls = none.calls;
  // IVF-Flat: the largest row norm of the survivors, as a fresh build has it (the pad rows are zeros).  Last: nothing after it can fail
  // but the wait.
  if (!ix->pq.m && !ix->sq.on) {
    HIPCHK(hipMemsetAsync(ix->flat.maxnorm, 0, sizeof(int), ix->stream));
    HIPCHK(launch_maxnorm(G.rows, G.prow, ix->d, ix->flat.maxnorm, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
  }
  if ((r = ivf_swap_in(ix, G.L, G.work, G.pq_codes, G.sq_codes, G.rows, G.tile0, G.size, G.prow, G.ntotal))) return r;
  ix->shrink = G.stats;
  if (n_removed) *n_removed = G.stats.n_removed;
  return KNNX_OK;
}

extern "C" int knnx_ivf_remove_stats(knnx_index* ix, double* mark_ms, double* plan_ms, double* move_ms, double* ids_ms, int64_t* moved_bytes,
                                     int64_t* n_removed) {
  if (!ix) return fail(KNNX_E_ARG, "knnx_ivf_remove_stats: index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->shrink.calls) return fail(KNNX_E_STATE, "knnx_ivf_remove_stats: nothing has been removed from the index yet");
  if (mark_ms) *mark_ms = ix->shrink.mark_ms;
  if (plan_ms) *plan_ms = ix->shrink.plan_ms;
  if (move_ms) *move_ms = ix->shrink.move_ms;
  if (ids_ms) *ids_ms = ix->shrink.ids_ms;
  if (moved_bytes) *moved_bytes = ix->shrink.moved_bytes;
  if (n_removed) *n_removed = ix->shrink.n_removed;
  return KNNX_OK;
}
