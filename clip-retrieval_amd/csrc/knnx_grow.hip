// knnx_grow.hip -- growing a BUILT IVF index of any kind (IVF-Flat, IVF-PQ with its rotation / refine store / M = 256 / threshold scan,
// IVF-SQ8): knnx_ivf_append_assigned / knnx_ivf_append / knnx_ivf_append_device / knnx_ivf_merge_from (include/knnx.h, "Growing a built
// index").  The host plan is knnx_grow_plan.h, the move kernels knn_grow_kernels.hip.
//
// Every call is OUT OF PLACE and all or nothing: the new layout, id maps and arenas are allocated and filled next to the old ones -- the
// occupied tiles moved by launch_ivf_grow_move, the new rows scattered / encoded by the kernels of the build -- and only when all of that
// has succeeded does grow_commit() swap them into the index, under knnx_index::mu and IdOrder::mu.  A search from another thread sees the
// index before or after the call; a failure (an allocation above all) leaves it exactly as it was.  Whatever caches the layout is
// refreshed or dropped by ivf_swap_in(), in one place, which grow_commit() and the removal of ids (knnx_shrink.hip) both call.

#include <chrono>

#include "knnx_host.h"
#include "knnx_grow_plan.h"

namespace {

// the state a call builds next to the index
struct Grown {
  GrowPlan plan;
  IvfLayout L;
  DevBuf<uint4> work;           // ivf1.work of the new tile count
  DevBuf<_Float16> rows;        // IVF-Flat rows / the refine store
  DevBuf<uint8_t> pq_codes, sq_codes;
  DevBuf<uint32_t> src_tile;
  int64_t ntotal = 0;           // rows of the grown index
  Event ev_move0, ev_copy1, ev_move1, ev_fill;  // around the move (payload | ids), after the last scatter / encode kernel (knnx_ivf_grow_stats)
  GrowStats stats;
};

// staging of one chunk of appended rows
struct Stage {
  int64_t cap = 0;
  DevBuf<_Float16> rows;   // [cap, d] rows that came from the host
  DevBuf<_Float16> rot;    // [cap, d_out] the chunk rotated (an index with a rotation)
  DevBuf<_Float16> rot_w;  // the hi / lo tile image of the rotation, as knnx_ivfpq_set_rotation made it (knnx_ivf_end released it)
  DevBuf<int32_t> lists, pos;
  DevBuf<int64_t> ids;     // merge only
  int64_t staged_o = -1;   // the chunk of host rows `rows` holds
};

int hip_fail(const char* who, hipError_t e) {
  (void)hipGetLastError();
  return fail(e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

// an index that can grow: built, IVF, owning its rows
int grow_refuse(const knnx_index* ix, const char* who) {
  if (ix->ivfb.nlist)
    return fail(KNNX_E_ARG, std::string(who) + ": the index is between knnx_ivf_begin and knnx_ivf_end (finish the build first; nothing was added)");
  if (!ix->ivf_nlist || !ix->cent) return fail(KNNX_E_ARG, std::string(who) + ": not a built IVF index (nothing was added)");
  if (ix->rows.borrowed) return fail(KNNX_E_ARG, std::string(who) + ": the index borrows its rows (nothing was added)");
  return 0;
}

int download_sizes(knnx_index* ix, std::vector<unsigned>& size) {
  size.resize((size_t)ix->ivf_nlist);
  HIPCHK(hipStreamSynchronize(ix->stream));
  HIPCHK(hipMemcpy(size.data(), ix->ivf.size, size.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
  return 0;
}

// plan, allocate and move: after this G holds the grown index without the new rows (their slots are zero, idmap -1), queued on ix->stream
int grow_open(knnx_index* ix, const char* who, const std::vector<unsigned>& size_old, const std::vector<int64_t>& extra, int64_t n_new, Grown& G) {
  const int nlist = ix->ivf_nlist;
  const int pr = grow_plan(nlist, size_old.data(), extra.data(), G.plan);
  if (pr == GROW_E_ROWS) return fail(KNNX_E_UNSUPPORTED, std::string(who) + ": more than 2^32 padded rows per device (nothing was added)");
  if (pr) return fail(KNNX_E_ARG, std::string(who) + ": negative list size");
  const GrowPlan& P = G.plan;
  if (P.old_rows != ix->ntotal || std::max<int64_t>(P.old_tiles * 32, 32) != ix->capacity)
    return fail(KNNX_E_STATE, std::string(who) + ": internal: the list sizes do not add up to the index");
  G.ntotal = ix->ntotal + n_new;
  if (P.rows != G.ntotal) return fail(KNNX_E_STATE, std::string(who) + ": internal: the plan does not hold the new rows");
  const size_t nl = (size_t)nlist, prow = (size_t)P.prow, ntab = P.src_tile.size();
  hipError_t e = hipSuccess;
  dev_alloc(e, G.L.tile0, nl);
  dev_alloc(e, G.L.ntile, nl);
  dev_alloc(e, G.L.size, nl);
  dev_alloc(e, G.L.idmap, prow);
  dev_alloc(e, G.L.inv, (size_t)std::max<int64_t>(P.rows, 1));
  dev_alloc(e, G.work, (size_t)std::max<int64_t>(P.tiles, 1));
  dev_alloc(e, G.src_tile, ntab);
  if (ix->pq.m) dev_alloc(e, G.pq_codes, prow * (size_t)ix->pq.m);
  if (ix->sq.on) dev_alloc(e, G.sq_codes, prow * (size_t)ix->d);
  if ((!ix->pq.m && !ix->sq.on) || ix->pq.refine) dev_alloc(e, G.rows, prow * (size_t)ix->d);
  hipStream_t st = ix->stream;
  if (e == hipSuccess) e = hipMemcpyAsync(G.L.tile0, P.tile0.data(), nl * sizeof(unsigned), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(G.L.ntile, P.ntile.data(), nl * sizeof(unsigned), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(G.L.size, P.size.data(), nl * sizeof(unsigned), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(G.src_tile, P.src_tile.data(), ntab * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  // (the arena of an index without a tile still has one: prow = 32, and the table one entry)
  const int64_t tiles = P.prow / 32;
  if (e == hipSuccess) e = G.ev_move0.create();
  if (e == hipSuccess) e = G.ev_move1.create();
  if (e == hipSuccess) e = G.ev_copy1.create();
  if (e == hipSuccess) e = G.ev_fill.create();
  if (e == hipSuccess) e = hipEventRecord(G.ev_move0, st);
  G.stats.moved_bytes = P.moved_tiles * 32 * ((G.pq_codes ? (int64_t)ix->pq.m : 0) + (G.sq_codes ? (int64_t)ix->d : 0) + (G.rows ? (int64_t)2 * ix->d : 0));
  if (e == hipSuccess && G.pq_codes) e = launch_ivf_grow_move(ix->pq.codes, G.pq_codes, ix->pq.m, G.src_tile, tiles, ix->n_cu, st);
  if (e == hipSuccess && G.sq_codes) e = launch_ivf_grow_move(ix->sq.codes, G.sq_codes, ix->d, G.src_tile, tiles, ix->n_cu, st);
  if (e == hipSuccess && G.rows) e = launch_ivf_grow_move(ix->rows, G.rows, 2 * ix->d, G.src_tile, tiles, ix->n_cu, st);
  if (e == hipSuccess) e = hipEventRecord(G.ev_copy1, st);
  if (e == hipSuccess) e = launch_ivf_grow_ids(ix->ivf.idmap, G.src_tile, P.prow, ix->id_base, G.ntotal, G.L.idmap, G.L.inv, st);
  if (e == hipSuccess) e = hipEventRecord(G.ev_move1, st);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    return hip_fail(who, e);
  }
  return 0;
}

// the grown state becomes the index (ivf_swap_in, below the namespace), and the call's timings its grow stats.  The caller holds ix->mu
// and has synchronised ix->stream.
int grow_commit(knnx_index* ix, Grown& G) {
  float ms = 0;
  HIPCHK(hipEventRecord(G.ev_fill, ix->stream));
  HIPCHK(hipEventSynchronize(G.ev_fill));
  HIPCHK(hipEventElapsedTime(&ms, G.ev_move0, G.ev_move1));
  G.stats.move_ms = ms;
  HIPCHK(hipEventElapsedTime(&ms, G.ev_copy1, G.ev_move1));
  G.stats.ids_ms = ms;
  HIPCHK(hipEventElapsedTime(&ms, G.ev_move1, G.ev_fill));
  G.stats.fill_ms = ms;
  G.stats.calls = ix->grow.calls + 1;
  int r = ivf_swap_in(ix, G.L, G.work, G.pq_codes, G.sq_codes, G.rows, G.plan.tile0, G.plan.size, G.plan.prow, G.ntotal);
  if (r) return r;
  ix->grow = G.stats;
  return 0;
}

int stage_alloc(knnx_index* ix, const char* who, int64_t n, bool host_rows, bool merge, Stage& S) {
  S.cap = std::min<int64_t>(std::max<int64_t>(n, 1), IVFB_CHUNK);
  const int dq = ix->pq.m ? pq_dq(ix) : ix->d;
  hipError_t e = hipSuccess;
  if (host_rows) dev_alloc(e, S.rows, (size_t)S.cap * ix->d);
  if (!merge && ix->pq.rot) {
    dev_alloc(e, S.rot, (size_t)S.cap * dq);
    dev_alloc(e, S.rot_w, (size_t)2 * dq * ix->d);
    if (e == hipSuccess) e = launch_rot_split(ix->pq.rot, ix->d, dq, S.rot_w, ix->stream);
  }
  dev_alloc(e, S.lists, (size_t)S.cap);
  dev_alloc(e, S.pos, (size_t)S.cap);
  if (merge) dev_alloc(e, S.ids, (size_t)S.cap);
  if (e != hipSuccess) return hip_fail(who, e);
  return 0;
}

// rows [o, o + m) of the call on the device: where they are, or staged through the pinned buffer
int fetch_rows(knnx_index* ix, const uint16_t* rows_host, const void* rows_dev, int64_t o, int64_t m, Stage& S, const _Float16** out) {
  if (rows_dev) {
    *out = (const _Float16*)rows_dev + (size_t)o * ix->d;
    return 0;
  }
  *out = S.rows;
  if (S.staged_o == o) return 0;
  const size_t bytes = (size_t)m * ix->d * sizeof(_Float16);
  int r = ensure_pin(ix, bytes);
  if (r) return r;
  memcpy(ix->pin.p, rows_host + (size_t)o * ix->d, bytes);
  HIPCHK(hipMemcpyAsync(S.rows, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->stream));
  HIPCHK(hipStreamSynchronize(ix->stream));
  S.staged_o = o;
  return 0;
}

// rows -> their place in the grown state; lists_h [n]: the list of every row (checked by the caller)
int append_rows(knnx_index* ix, const uint16_t* rows_host, const void* rows_dev, int64_t n, const int32_t* lists_h,
                const std::vector<unsigned>& size_old, Stage& S, Grown& G) {
  hipStream_t st = ix->stream;
  const int d = ix->d, dq = ix->pq.m ? pq_dq(ix) : ix->d;
  std::vector<int64_t> cursor(size_old.begin(), size_old.end());
  std::vector<int32_t> pos((size_t)S.cap);
  for (int64_t o = 0; o < n; o += S.cap) {
    const int64_t m = std::min(S.cap, n - o);
    const _Float16* src = nullptr;
    int r = fetch_rows(ix, rows_host, rows_dev, o, m, S, &src);
    if (r) return r;
    if (grow_positions(ix->ivf_nlist, lists_h + o, m, cursor, pos.data())) return fail(KNNX_E_STATE, "internal: list id out of range after the check");
    HIPCHK(hipMemcpyAsync(S.lists, lists_h + o, (size_t)m * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S.pos, pos.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    const int64_t id0 = ix->id_base + ix->ntotal + o;
    if (ix->pq.m) {
      if (ix->pq.refine)
        HIPCHK(launch_ivf_scatter(src, m, d, S.lists, S.pos, nullptr, id0, G.L.tile0, ix->id_base, G.ntotal, G.rows, G.L.idmap, G.L.inv, st));
      if (ix->pq.rot) HIPCHK(launch_rotate_f16(S.rot_w, d, dq, src, m, S.rot, st));
      // (the centroids of the encoder: the rows of the coarse index, fp16 [nlist][d_out] as knnx_ivf_begin was given them)
      HIPCHK(launch_pq_encode(ix->pq.rot ? S.rot.p : src, m, dq, ix->pq.m, S.lists, ix->cent->rows, ix->pq.cb, G.L.tile0, S.pos, nullptr, id0,
                              ix->id_base, G.ntotal, G.pq_codes, G.L.idmap, G.L.inv, st));
    } else if (ix->sq.on) {
      HIPCHK(launch_sq_encode(src, m, d, S.lists, S.pos, nullptr, id0, G.L.tile0, ix->id_base, G.ntotal, ix->sq.vmin, ix->sq.scale, G.sq_codes,
                              G.L.idmap, G.L.inv, st));
    } else {
      HIPCHK(launch_ivf_scatter(src, m, d, S.lists, S.pos, nullptr, id0, G.L.tile0, ix->id_base, G.ntotal, G.rows, G.L.idmap, G.L.inv, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // (pos is reused by the next chunk)
  }
  if (!ix->pq.m && !ix->sq.on)  // IVF-Flat: the largest row norm, last -- nothing after it can fail but the wait
    for (int64_t o = 0; o < n; o += S.cap) {
      const int64_t m = std::min(S.cap, n - o);
      const _Float16* src = nullptr;
      int r = fetch_rows(ix, rows_host, rows_dev, o, m, S, &src);
      if (r) return r;
      HIPCHK(launch_maxnorm(src, m, d, ix->flat.maxnorm, st));
      HIPCHK(hipStreamSynchronize(st));
    }
  return 0;
}

int append_common(knnx_index* ix, const char* who, const uint16_t* rows_host, const void* rows_dev, int64_t n, const int32_t* lists_in,
                  int32_t* lists_out) {
  if (!ix) return fail(KNNX_E_ARG, std::string(who) + ": index is null");
  if (n < 0 || (n > 0 && !rows_host && !rows_dev)) return fail(KNNX_E_ARG, std::string(who) + ": bad arguments (nothing was added)");
  std::lock_guard<std::mutex> lk(ix->mu);
  int r = grow_refuse(ix, who);
  if (r) return r;
  if (n == 0) return KNNX_OK;
  if (set_dev(ix)) return KNNX_E_HIP;
  const int nlist = ix->ivf_nlist, d = ix->d, dq = ix->pq.m ? pq_dq(ix) : ix->d;
  if (lists_in)  // checked before the device is touched
    for (int64_t i = 0; i < n; ++i)
      if (lists_in[i] < 0 || lists_in[i] >= nlist) return fail(KNNX_E_ARG, std::string(who) + ": list id out of range (nothing was added)");
  hipStream_t st = ix->stream;
  if ((r = scratch_acquire(ix, st))) return r;
  Stage S;
  if ((r = stage_alloc(ix, who, n, rows_host != nullptr, false, S))) return r;
  std::vector<int32_t> assigned;
  double assign_ms = 0;
  std::chrono::steady_clock::time_point t_assign0;
  if (!lists_in) {  // the library assigns: the MFMA assignment kernel over the index's own centroids, in the quantiser space
    assigned.resize((size_t)n);
    t_assign0 = std::chrono::steady_clock::now();
    for (int64_t o = 0; o < n; o += S.cap) {
      const int64_t m = std::min(S.cap, n - o);
      const _Float16* src = nullptr;
      if ((r = fetch_rows(ix, rows_host, rows_dev, o, m, S, &src))) return r;
      if (ix->pq.rot) HIPCHK(launch_rotate_f16(S.rot_w, d, dq, src, m, S.rot, st));
      HIPCHK(launch_assign(ix->cent->rows, nlist, dq, ix->pq.rot ? S.rot.p : src, m, S.lists, st));
      HIPCHK(hipMemcpyAsync(assigned.data() + o, S.lists, (size_t)m * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    lists_in = assigned.data();
    assign_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_assign0).count();
  }
  std::vector<int64_t> extra((size_t)nlist, 0);
  if (grow_count(nlist, lists_in, n, extra)) return fail(KNNX_E_ARG, std::string(who) + ": list id out of range (nothing was added)");
  std::vector<unsigned> size_old;
  if ((r = download_sizes(ix, size_old))) return r;
  Grown G;
  if ((r = grow_open(ix, who, size_old, extra, n, G))) return r;
  G.stats.assign_ms = assign_ms;
  if ((r = append_rows(ix, rows_host, rows_dev, n, lists_in, size_old, S, G))) return r;
  HIPCHK(hipStreamSynchronize(st));
  if ((r = grow_commit(ix, G))) return r;
  if (lists_out) memcpy(lists_out, lists_in, (size_t)n * sizeof(int32_t));
  return KNNX_OK;
}

// what knnx_ivf_merge_from takes out of `other` under other's lock
struct MergeSrc {
  int kind = 0;  // 0 IVF-Flat, 1 IVF-PQ, 2 IVF-SQ8
  int d = 0, dq = 0, nlist = 0, m = 0, device = 0;
  bool refine = false;
  int64_t ntotal = 0, id_base = 0;
  std::vector<uint16_t> cent;
  std::vector<float> cb, rot, vmin, vdiff;
  std::vector<int64_t> ids;
  std::vector<int32_t> lists;
  std::vector<uint8_t> codes, rows;  // arena order: list by list, a list's rows in their own order
};

int ix_kind(const knnx_index* ix) { return ix->pq.m ? 1 : ix->sq.on ? 2 : 0; }

// the quantisers of an index on the host (centroids, codebooks; rotation and ranges are kept on the host by the index)
int quantisers(knnx_index* ix, std::vector<uint16_t>& cent, std::vector<float>& cb) {
  const int dq = ix->pq.m ? pq_dq(ix) : ix->d;
  HIPCHK(hipStreamSynchronize(ix->cent->stream));
  cent.resize((size_t)ix->ivf_nlist * dq);
  HIPCHK(hipMemcpy(cent.data(), ix->cent->rows, cent.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
  cb.clear();
  if (ix->pq.m) {
    cb.resize((size_t)256 * dq);
    HIPCHK(hipMemcpy(cb.data(), ix->pq.cb, cb.size() * sizeof(float), hipMemcpyDeviceToHost));
  }
  return 0;
}

template <class T>
bool bits_equal(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

}  // namespace

// A layout built next to the index -- by a call that grew it (above) or shrank it (knnx_shrink.hip) -- becomes the index.  Everything
// that caches the layout is refreshed or dropped HERE; nprobe, k_factor, the refine and threshold-scan switches and every counter stay.
// The caller holds ix->mu and has synchronised ix->stream; the old buffers leave in the arguments (hipFree waits for the device, so a
// search_device still queued on a caller's stream finishes on the arena it was launched on).  A payload the index does not have is null.
int ivf_swap_in(knnx_index* ix, IvfLayout& L, DevBuf<uint4>& work, DevBuf<uint8_t>& pq_codes, DevBuf<uint8_t>& sq_codes, DevBuf<_Float16>& rows,
                const std::vector<unsigned>& tile0_h, const std::vector<unsigned>& size_h, int64_t prow, int64_t ntotal) {
  IdOrder& S = ix->ido;
  std::lock_guard<std::mutex> lk(S.mu);  // a translation of ids (knnx_ivf_map_ids) reads the layout without ix->mu
  if (S.stream) HIPCHK(hipStreamSynchronize(S.stream));
  std::swap(ix->ivf, L);
  std::swap(ix->ivf1.work, work);
  if (pq_codes) std::swap(ix->pq.codes, pq_codes);
  if (sq_codes) std::swap(ix->sq.codes, sq_codes);
  if (rows) std::swap(ix->rows, rows);
  ix->capacity = prow;
  ix->ntotal = ntotal;
  // the multi-block scratch is sized by the tiles of the arena and allocated once: drop it, the next pass allocates it for the new size
  ix->ivfm = IvfMultiScratch();
  ix->ivfm_last_blk = 0;
  ix->ivfm_union_valid = false;
  if (ix->pq.m) {
    ix->pq.tile0_h.assign(tile0_h.begin(), tile0_h.end());
    ix->pq.size_h.assign(size_h.begin(), size_h.end());
    ix->pq.slab_np = 0;  // (M = 256: the slab width follows the list sizes)
    ix->pq.slab = 0;
    ix->pq.thr.tthr.reset(), ix->pq.thr.tcnt.reset(), ix->pq.thr.tfetch.reset();
  }
  if (ix->sq.on) {
    ix->sq.tile0_h.assign(tile0_h.begin(), tile0_h.end());
    ix->sq.size_h.assign(size_h.begin(), size_h.end());
    ix->sq.thr.tthr.reset(), ix->sq.thr.tcnt.reset(), ix->sq.thr.tfetch.reset();
  }
  // per-pass scratch of the compressed scans (probe offsets and partial sums of a pass over the old layout) and the hit pools
  ix->pqs = PqScratch();
  ix->sqs = SqScratch();
  ix->range = RangePools();
  // the list-order cache: dense0 is rebuilt by the next translation
  S.ready = false;
  S.dense0.reset();
  S.dense0_h.clear();
  return 0;
}

extern "C" int knnx_ivf_append_assigned(knnx_index* ix, const uint16_t* rows_f16, int64_t n, const int32_t* lists) {
  if (ix && n > 0 && !lists) return fail(KNNX_E_ARG, "knnx_ivf_append_assigned: lists is null (nothing was added)");
  return append_common(ix, "knnx_ivf_append_assigned", rows_f16, nullptr, n, lists, nullptr);
}

extern "C" int knnx_ivf_append(knnx_index* ix, const uint16_t* rows_f16, int64_t n, int32_t* lists_out) {
  return append_common(ix, "knnx_ivf_append", rows_f16, nullptr, n, nullptr, lists_out);
}

extern "C" int knnx_ivf_append_device(knnx_index* ix, const void* rows_dev_f16, int64_t n, int32_t* lists_out) {
  return append_common(ix, "knnx_ivf_append_device", nullptr, rows_dev_f16, n, nullptr, lists_out);
}

extern "C" int knnx_ivf_merge_from(knnx_index* ix, knnx_index* other) {
  const char* who = "knnx_ivf_merge_from";
  if (!ix || !other) return fail(KNNX_E_ARG, std::string(who) + ": index is null");
  if (ix == other) return fail(KNNX_E_ARG, std::string(who) + ": an index cannot be merged into itself (nothing was added)");
  MergeSrc M;
  int r;
  {  // ---- other, under its own lock: its description and every row in arena order, staged on the host.  It is left untouched.
    std::lock_guard<std::mutex> lk(other->mu);
    if ((r = grow_refuse(other, "knnx_ivf_merge_from (other)"))) return r;
    if (set_dev(other)) return KNNX_E_HIP;
    M.kind = ix_kind(other), M.d = other->d, M.dq = other->pq.m ? pq_dq(other) : other->d, M.nlist = other->ivf_nlist, M.m = other->pq.m;
    M.device = other->device, M.refine = other->pq.refine, M.ntotal = other->ntotal, M.id_base = other->id_base;
    M.rot = other->pq.rot_h, M.vmin = other->sq.vmin_h, M.vdiff = other->sq.vdiff_h;
    if ((r = quantisers(other, M.cent, M.cb))) return r;
    std::vector<unsigned> size_h, tile0_h((size_t)M.nlist);
    if ((r = download_sizes(other, size_h))) return r;
    HIPCHK(hipMemcpy(tile0_h.data(), other->ivf.tile0, tile0_h.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    const size_t n = (size_t)M.ntotal;
    M.ids.resize(n), M.lists.resize(n);
    if (M.kind == 1) {
      M.codes.resize(n * (size_t)M.m);
      if ((r = ivf_export_codes_locked(other, other->pq.codes, M.m, tile0_h, size_h, "IVF-PQ", M.ids.data(), M.lists.data(), M.codes.data()))) return r;
    } else if (M.kind == 2) {
      M.codes.resize(n * (size_t)M.d);
      if ((r = ivf_export_codes_locked(other, other->sq.codes, M.d, tile0_h, size_h, "IVF-SQ8", M.ids.data(), M.lists.data(), M.codes.data()))) return r;
    }
    if (M.kind == 0 || M.refine) {
      M.rows.resize(n * (size_t)M.d * 2);
      if ((r = ivf_export_codes_locked(other, (const uint8_t*)other->rows.p, 2 * M.d, tile0_h, size_h, "IVF", M.ids.data(), M.lists.data(),
                                       M.rows.data())))
        return r;
    }
  }
  // ---- ix: compare, then grow
  std::lock_guard<std::mutex> lk(ix->mu);
  if ((r = grow_refuse(ix, who))) return r;
  if (set_dev(ix)) return KNNX_E_HIP;
  static const char* kinds[3] = {"IVF-Flat", "IVF-PQ", "IVF-SQ8"};
  const auto differ = [&](const std::string& what) { return fail(KNNX_E_ARG, std::string(who) + ": the indexes differ in " + what + " (nothing was added)"); };
  if (ix_kind(ix) != M.kind) return differ(std::string("kind (") + kinds[ix_kind(ix)] + " and " + kinds[M.kind] + ")");
  const int dq = ix->pq.m ? pq_dq(ix) : ix->d;
  if (ix->d != M.d) return differ("d");
  if (dq != M.dq) return differ("d_out");
  if (ix->ivf_nlist != M.nlist) return differ("nlist");
  if (ix->pq.m != M.m) return differ("M");
  if (ix->pq.refine != M.refine) return differ("the refine store (one has it, the other has not)");
  {
    std::vector<uint16_t> cent;
    std::vector<float> cb;
    if ((r = quantisers(ix, cent, cb))) return r;
    if (!bits_equal(cent, M.cent)) return differ("centroids");
    if (!bits_equal(cb, M.cb)) return differ("codebooks");
    if (!bits_equal(ix->pq.rot_h, M.rot)) return differ("rotation");
    if (!bits_equal(ix->sq.vmin_h, M.vmin) || !bits_equal(ix->sq.vdiff_h, M.vdiff)) return differ("ranges (vmin / vdiff)");
  }
  const int64_t n = M.ntotal;
  if (n == 0) return KNNX_OK;
  const int nlist = ix->ivf_nlist, d = ix->d;
  for (int64_t i = 0; i < n; ++i)
    if (M.ids[i] < M.id_base || M.ids[i] - M.id_base >= n) return fail(KNNX_E_STATE, std::string(who) + ": internal: other's ids are not a dense range");
  hipStream_t st = ix->stream;
  if ((r = scratch_acquire(ix, st))) return r;
  Stage S;
  if ((r = stage_alloc(ix, who, n, false, true, S))) return r;
  const size_t cw = M.kind == 1 ? (size_t)M.m : M.kind == 2 ? (size_t)d : 0, rw = (M.kind == 0 || M.refine) ? (size_t)2 * d : 0;
  DevBuf<uint8_t> stage;  // one chunk of codes or of rows
  HIPCHK(stage.alloc((size_t)S.cap * std::max(cw, rw)));
  std::vector<int64_t> extra((size_t)nlist, 0);
  if (grow_count(nlist, M.lists.data(), n, extra)) return fail(KNNX_E_STATE, std::string(who) + ": internal: other's list ids are out of range");
  std::vector<unsigned> size_old;
  if ((r = download_sizes(ix, size_old))) return r;
  Grown G;
  if ((r = grow_open(ix, who, size_old, extra, n, G))) return r;
  // other's row with id j gets id id_base + ntotal + (j - other's id_base); inside a list the rows keep other's order (the arena order
  // of the export), behind the rows already there.  Codes and rows are copied, never encoded again.
  std::vector<int64_t> cursor(size_old.begin(), size_old.end()), ids((size_t)S.cap);
  std::vector<int32_t> pos((size_t)S.cap);
  for (int64_t o = 0; o < n; o += S.cap) {
    const int64_t m = std::min(S.cap, n - o);
    if (grow_positions(nlist, M.lists.data() + o, m, cursor, pos.data())) return fail(KNNX_E_STATE, "internal: list id out of range after the check");
    for (int64_t i = 0; i < m; ++i) ids[(size_t)i] = ix->id_base + ix->ntotal + (M.ids[(size_t)(o + i)] - M.id_base);
    HIPCHK(hipMemcpyAsync(S.ids, ids.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S.lists, M.lists.data() + o, (size_t)m * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S.pos, pos.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    if (cw) {
      HIPCHK(hipMemcpyAsync(stage, M.codes.data() + (size_t)o * cw, (size_t)m * cw, hipMemcpyHostToDevice, st));
      HIPCHK(launch_pq_scatter_codes(stage, m, (int)cw, S.lists, S.pos, S.ids, G.L.tile0, ix->id_base, G.ntotal, M.kind == 1 ? G.pq_codes.p : G.sq_codes.p,
                                     G.L.idmap, G.L.inv, st));
    }
    if (rw) {
      HIPCHK(hipMemcpyAsync(stage, M.rows.data() + (size_t)o * rw, (size_t)m * rw, hipMemcpyHostToDevice, st));
      HIPCHK(launch_ivf_scatter((const _Float16*)stage.p, m, d, S.lists, S.pos, S.ids, 0, G.L.tile0, ix->id_base, G.ntotal, G.rows, G.L.idmap, G.L.inv, st));
      if (M.kind == 0) HIPCHK(launch_maxnorm((const _Float16*)stage.p, m, d, ix->flat.maxnorm, st));
    }
    HIPCHK(hipStreamSynchronize(st));
  }
  return grow_commit(ix, G);
}

extern "C" int knnx_ivf_grow_stats(knnx_index* ix, double* assign_ms, double* move_ms, double* ids_ms, double* fill_ms, int64_t* moved_bytes) {
  if (!ix) return fail(KNNX_E_ARG, "knnx_ivf_grow_stats: index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->grow.calls) return fail(KNNX_E_STATE, "knnx_ivf_grow_stats: the index has not grown yet");
  if (assign_ms) *assign_ms = ix->grow.assign_ms;
  if (move_ms) *move_ms = ix->grow.move_ms;
  if (ids_ms) *ids_ms = ix->grow.ids_ms;
  if (fill_ms) *fill_ms = ix->grow.fill_ms;
  if (moved_bytes) *moved_bytes = ix->grow.moved_bytes;
  return KNNX_OK;
}
