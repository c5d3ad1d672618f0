"""faiss-`Index`-shaped object over the MI355X kNN library (search half of the hot path).

Mirrors exactly the part of the faiss Index API the reference exercises:
  * `search_and_reconstruct(x, k) -> (D, I, R)`   clip_retrieval/clip_back.py:362
  * `search(x, k) -> (D, I)`                      clip_retrieval/clip_filter.py:55
  * `range_search(x, thresh) -> (lims, D, I)`     clip_retrieval/clip_filter.py:52, clip_back.py:294
  * `.ntotal`, `.d`, `add(x)`, `reconstruct(i)`   ivf_metadata_ordering.py:51, clip_back.py:292-293
so an instance can be dropped into `ClipResource.image_index` / `.text_index` (clip_back.py:781-782).
`load_index` builds one from the `img_emb/*.npy` folder `clip inference` writes (writer.py:67-75),
taking the place of clip_back.py:589-596 for our index type.

Same argument meaning and error behaviour as faiss: float32 C-contiguous [n, d] queries (anything else
raises like faiss' SWIG wrapper does), int64 labels, -1 / -FLT_MAX padding, exceptions on misuse.
Thread-safe: clip_back serves each request on its own werkzeug thread with n=1 (clip_back.py:1018);
concurrent callers are coalesced into one HBM scan of up to 256 queries (_SCAN_QUERIES) by a leader/follower batcher.
"""

import ctypes as C
import glob
import os
import threading

import numpy as np

from ._lib import HipLibraryError, check, load_library

METRIC_INNER_PRODUCT = 0
_SCAN_QUERIES = 256  # queries one HBM scan serves at most (KNN_RQ_MAX in csrc/knn_kernels.h: the RQ scan; 64: the wide scan)


def _as_queries(x, d):
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise TypeError(f"queries must be float32 (got {x.dtype}); faiss raises the same way")
    if x.ndim != 2 or x.shape[1] != d:
        raise AssertionError(f"queries must have shape [n, {d}], got {x.shape}")
    return np.ascontiguousarray(x)


def _map_ids_call(lib, fn, handle, ids):
    """ids of any shape (int64) through knnx_ivf_map_ids / knnx_shards_map_ids -> a new int64 array of the same shape."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    out = np.empty_like(ids)
    check(lib, fn(handle, ids.ctypes.data, ids.size, out.ctypes.data), "knnx")
    return out


def _threshold_scan_property(family, handles, doc):
    """The property {pq,sq}_threshold_scan of an index class over knnx_{family}_threshold_scan / knnx_{family}_set_threshold_scan.
    handles(self) iterates over the native handles: the first is read, all are set."""
    def get(self):
        h = next(handles(self), None)
        return bool(getattr(self._lib, f"knnx_{family}_threshold_scan")(h)) if h else False  # pylint: disable=protected-access

    def put(self, on):
        for h in handles(self):
            check(self._lib, getattr(self._lib, f"knnx_{family}_set_threshold_scan")(h, 1 if on else 0), "knnx")  # pylint: disable=protected-access

    return property(get, put, doc=doc)


def _threshold_stats(index, family):
    v = [C.c_int64(0) for _ in range(4)]
    check(index._lib, getattr(index._lib, f"knnx_{family}_threshold_stats")(index._h, *[C.byref(x) for x in v]), "knnx")  # pylint: disable=protected-access
    return tuple(int(x.value) for x in v)


def _own_handle(index):
    return iter((index._h,))  # pylint: disable=protected-access


def _shard_handles(index):
    return (C.c_void_p(index._lib.knnx_shards_get(index._h, g)) for g in range(index.nshards))  # pylint: disable=protected-access


class _FaissShaped:
    """The part of the faiss Index surface clip_back / clip_filter exercise, on top of `_search_raw`,
    `reconstruct_batch`, `range_search` and `ntotal` of the concrete index (one GPU or row-sharded)."""

    def _init_queue(self, coalesce):
        self._coalesce = coalesce
        self._q_lock = threading.Lock()
        self._pending = []  # [(k, want_r, query_row, slot)]
        self._leader_active = False

    def _search_coalesced(self, q, k, want_r):
        """n == 1 callers from many threads: the first becomes the leader and serves every query queued
        while the GPU was busy, up to one scan's worth, in a single pass over HBM."""
        slot = {"ev": threading.Event(), "out": None, "err": None}
        with self._q_lock:
            self._pending.append((k, want_r, q[0], slot))
            lead = not self._leader_active
            if lead:
                self._leader_active = True
        if not lead:
            slot["ev"].wait()
        else:
            while True:
                with self._q_lock:
                    if not self._pending:
                        self._leader_active = False
                        break
                    k0, r0 = self._pending[0][0], self._pending[0][1]
                    take = [p for p in self._pending if p[0] == k0 and p[1] == r0][:_SCAN_QUERIES]
                    taken = set(id(p) for p in take)
                    self._pending = [p for p in self._pending if id(p) not in taken]
                try:
                    qq = np.stack([p[2] for p in take]).astype(np.float32)
                    D, I, R = self._search_raw(qq, k0, r0)
                    for j, p in enumerate(take):
                        p[3]["out"] = (D[j:j + 1], I[j:j + 1], R[j:j + 1] if R is not None else None)
                except Exception as e:  # pylint: disable=broad-except
                    for p in take:
                        p[3]["err"] = e
                for p in take:
                    p[3]["ev"].set()
        if slot["err"] is not None:
            raise slot["err"]
        return slot["out"]

    def _do_search(self, x, k, want_r):
        if k <= 0:
            raise AssertionError("k must be positive")
        q = _as_queries(x, self.d)
        if q.shape[0] == 0:
            return (np.empty((0, k), np.float32), np.empty((0, k), np.int64),
                    np.empty((0, k, self.d), np.float32) if want_r else None)
        if self._coalesce and q.shape[0] == 1:
            return self._search_coalesced(q, int(k), want_r)
        return self._search_raw(q, int(k), want_r)

    def search(self, x, k):
        D, I, _ = self._do_search(x, k, False)
        return D, I

    def search_and_reconstruct(self, x, k):
        return self._do_search(x, k, True)

    def reconstruct(self, key):
        return self.reconstruct_batch(np.asarray([key], dtype=np.int64))[0]

    def _pad(self, x):
        if self._dpad == self.d:
            return x
        out = np.zeros((x.shape[0], self._dpad), dtype=x.dtype)
        out[:, : self.d] = x
        return out

    def __del__(self):
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass


class Mi355xIndex(_FaissShaped):
    """Flat inner-product index with fp16 rows resident in HBM (one GPU)."""

    def __init__(self, d, device=0, id_base=0, coalesce=True):
        self._lib = load_library()
        self.d = int(d)
        self._dpad = (self.d + 255) // 256 * 256  # kernels want d % 256 == 0; extra columns are zeros
        self.device = int(device)
        h = C.c_void_p()
        check(self._lib, self._lib.knnx_create(self.device, self._dpad, METRIC_INNER_PRODUCT, C.byref(h)), "knnx")
        self._h = h
        self.metric_type = METRIC_INNER_PRODUCT
        self.is_trained = True
        self._id_base = int(id_base)
        if id_base:
            check(self._lib, self._lib.knnx_set_id_base(self._h, int(id_base)), "knnx")
        # concurrent single-query callers are coalesced INSIDE the library (knnx.h: knnx_set_coalesce; round 4 -- round 3 did it
        # here with a Python condition variable, and the GIL hand-offs capped a served index at 6.5 k requests/s)
        self._init_queue(False)
        check(self._lib, self._lib.knnx_set_coalesce(self._h, 1 if coalesce else 0), "knnx")

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.knnx_destroy(h)

    @property
    def ntotal(self):
        return int(self._lib.knnx_ntotal(self._h))

    # ------------------------------------------------------------------ building
    def reserve(self, n_rows):
        check(self._lib, self._lib.knnx_reserve(self._h, int(n_rows)), "knnx")

    def add(self, x):
        """faiss Index.add: float32 (rounded to fp16 on the device) or float16 rows."""
        x = np.asarray(x)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise AssertionError(f"add expects [n, {self.d}], got {x.shape}")
        if x.dtype == np.float16:
            x = np.ascontiguousarray(self._pad(x))
            check(self._lib, self._lib.knnx_add_f16(self._h, x.ctypes.data, x.shape[0]), "knnx")
        elif x.dtype == np.float32:
            x = np.ascontiguousarray(self._pad(x))
            check(self._lib, self._lib.knnx_add_f32(self._h, x.ctypes.data, x.shape[0]), "knnx")
        else:
            raise TypeError(f"add expects float32 or float16 rows, got {x.dtype}")

    def reset(self):
        """faiss Index.reset(): drop the rows, keep the HBM arena."""
        check(self._lib, self._lib.knnx_reset(self._h), "knnx")

    def attach_device_rows(self, dev_ptr, n_rows):
        """Borrow fp16 rows already in HBM (e.g. a torch tensor's data_ptr()); caller keeps them alive."""
        if self._dpad != self.d:
            raise HipLibraryError("attached rows must already be padded to a multiple of 256 columns")
        check(self._lib, self._lib.knnx_attach_device_f16(self._h, C.c_void_p(int(dev_ptr)), int(n_rows)), "knnx")

    def synth_fill(self, n_rows, seed):
        """Fill the index with the benchmark's synthetic corpus (oracle/knn_oracle.py:synth_rows)."""
        if self._dpad != self.d:
            raise HipLibraryError("synthetic fill needs d % 256 == 0")
        check(self._lib, self._lib.knnx_synth_fill(self._h, int(n_rows), C.c_uint64(int(seed))), "knnx")

    # ------------------------------------------------------------------ IVF-Flat
    def set_ivf_lists(self, centroids, list_sizes, ids):
        """Turn the index into a faiss-IndexIVFFlat-shaped one.  The rows must have been add()ed grouped by list;
        `centroids` [nlist, d] (stored fp16), `list_sizes` [nlist], `ids` [ntotal] = the id of every added row."""
        c = np.ascontiguousarray(self._pad(np.asarray(centroids).astype(np.float16)))
        sizes = np.ascontiguousarray(list_sizes, dtype=np.int64)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if c.shape[0] != sizes.shape[0] or ids.shape[0] != self.ntotal:
            raise AssertionError("centroids/list_sizes/ids disagree with the index")
        check(self._lib, self._lib.knnx_ivf_set_lists(self._h, c.shape[0], c.ctypes.data, sizes.ctypes.data, ids.ctypes.data), "knnx")

    @property
    def nlist(self):
        return int(self._lib.knnx_ivf_nlist(self._h))

    @property
    def nprobe(self):
        return int(self._lib.knnx_ivf_nprobe(self._h)) if self.nlist > 0 else getattr(self, "_nprobe", 1)

    @nprobe.setter
    def nprobe(self, v):
        """faiss `extract_index_ivf(index).nprobe = v` (clip_back.py:357-369)."""
        check(self._lib, self._lib.knnx_ivf_set_nprobe(self._h, int(v)), "knnx")
        self._nprobe = int(v)

    def last_scan_tiles(self):
        """IVF: 32-row tiles walked by the most recent scan (bytes read = tiles * 32 * d_padded * 2)."""
        t = C.c_int64(0)
        check(self._lib, self._lib.knnx_ivf_last_scan_tiles(self._h, C.byref(t)), "knnx")
        return int(t.value)

    def last_scan_union_tiles(self):
        """IVF: tiles of the union of the lists the most recent (multi-block) pass probed, each list counted once (profiling on)."""
        t = C.c_int64(0)
        check(self._lib, self._lib.knnx_ivf_last_scan_union_tiles(self._h, C.byref(t)), "knnx")
        return int(t.value)

    # ------------------------------------------------------------------ IVF-PQ
    def set_pq_quantizer(self, M, codebooks):
        """Make this EMPTY index an IVF-PQ one (faiss IndexIVFPQ(IndexFlatIP(d), d, nlist, M, 8)): codebooks f32 [M, 256, d_padded / M].
        M in {16, 32, 64, 128} dividing d_padded, or M = 256 (PQ256x8) with d_padded in {512, 768, 1024}; M = 256 scores in two halves of
        m through a scratch buffer of partial sums capped by KNNX_PQ_PARTIAL_MAX_BYTES (include/knnx.h).
        The rows then go in through knnx_ivf_begin / add_assigned / end (build_ivfpq_index*), which encode them."""
        cb = np.ascontiguousarray(codebooks, dtype=np.float32)
        dq = self._pq_width()  # (d_padded, or the d_out of set_pq_out_dim)
        if cb.size != 256 * dq:
            raise AssertionError(f"codebooks must hold M x 256 x d_padded / M = {256 * dq} floats, got {cb.shape}")
        check(self._lib, self._lib.knnx_ivfpq_set_quantizer(self._h, int(M), cb.ctypes.data), "knnx")

    def set_pq_out_dim(self, d_out):
        """Give this EMPTY index a quantiser space wider than its rows (faiss OPQMatrix(d, M, d_out), "OPQ256_768" on 512-d rows):
        before set_pq_quantizer, which then takes codebooks [M, 256, d_out / M]; the rotation is [d_out, d] and mandatory.  Both widths
        multiples of 256, 256 <= d < d_out <= 1024; d_out == d changes nothing (include/knnx.h: knnx_ivfpq_set_out_dim)."""
        d_out = int(d_out)
        if d_out != self.d and self.d % 256 != 0:
            raise ValueError(f"d_out = {d_out} != d needs d % 256 == 0 (got d = {self.d})")
        check(self._lib, self._lib.knnx_ivfpq_set_out_dim(self._h, d_out), "knnx")
        self._pq_dout = d_out if d_out != self.d else 0

    def _pq_width(self):
        """Width of the quantiser space as the library sees it: d_padded unless set_pq_out_dim gave a d_out."""
        return getattr(self, "_pq_dout", 0) or self._dpad

    @property
    def pq_out_dim(self):
        """Width of the quantiser space of an IVF-PQ index: d unless set_pq_out_dim gave another."""
        return getattr(self, "_pq_dout", 0) or self.d

    @property
    def pq_m(self):
        """Bytes of code per row of an IVF-PQ index (0: another index type)."""
        return int(self._lib.knnx_ivfpq_m(self._h)) if self._h else 0

    def pq_codebooks(self):
        """f32 [M, 256, d_padded / M]."""
        M = self.pq_m
        out = np.empty((M, 256, self._pq_width() // max(M, 1)), dtype=np.float32)
        check(self._lib, self._lib.knnx_ivfpq_get_codebooks(self._h, out.ctypes.data), "knnx")
        return out

    def set_pq_rotation(self, A):
        """OPQ rotation in front of this IVF-PQ index (faiss IndexPreTransform(OPQMatrix(d, M), IndexIVFPQ)): A f32 [d, d], y = A x,
        orthonormal (max |A A^T - I| <= 1e-3) or refused.  After set_pq_quantizer, before the rows go in.  Callers keep passing and
        receiving UN-ROTATED vectors: the index rotates rows and queries itself and reconstructs into the original space.
        After set_pq_out_dim(d_out): A f32 [d_out, d] with orthonormal columns (max |A^T A - I| <= 1e-3)."""
        A = np.asarray(A, dtype=np.float32)
        if A.shape != (self.pq_out_dim, self.d):
            raise AssertionError(f"the rotation must be [{self.pq_out_dim}, {self.d}], got {A.shape}")
        Ap = np.ascontiguousarray(A) if self.pq_out_dim != self.d else _pad_rotation(A, self._dpad)
        check(self._lib, self._lib.knnx_ivfpq_set_rotation(self._h, Ap.ctypes.data), "knnx")

    def pq_rotation(self):
        """The OPQ rotation f32 [d, d] ([d_out, d] after set_pq_out_dim), or None when the index has none."""
        out = np.empty((self._pq_width(), self._dpad), dtype=np.float32)
        rc = self._lib.knnx_ivfpq_get_rotation(self._h, out.ctypes.data)
        if rc == 1:
            return None
        check(self._lib, rc, "knnx")
        return np.ascontiguousarray(out[: self.pq_out_dim, : self.d])

    def set_pq_refine(self, on=True):
        """Refine store (faiss IndexRefineFlat(IndexIVFPQ)): the index keeps the fp16 rows next to the codes (2 d bytes more per row) and
        re-scores the k x k_factor best rows by ADC score exactly; reconstruct and the R of a search return the stored rows.  After
        set_pq_quantizer, before the rows go in (include/knnx.h: knnx_ivfpq_set_refine)."""
        check(self._lib, self._lib.knnx_ivfpq_set_refine(self._h, 1 if on else 0), "knnx")

    @property
    def pq_refine(self):
        """True when this IVF-PQ index has a refine store."""
        return bool(self._lib.knnx_ivfpq_refine(self._h)) if self._h else False

    @property
    def k_factor(self):
        """Candidates per result of a refine search (faiss IndexRefine.k_factor; 1 .. 512, k x k_factor <= 512)."""
        return int(self._lib.knnx_ivfpq_k_factor(self._h))

    @k_factor.setter
    def k_factor(self, v):
        check(self._lib, self._lib.knnx_ivfpq_set_k_factor(self._h, int(v)), "knnx")

    pq_threshold_scan = _threshold_scan_property("ivfpq", _own_handle, """The threshold mode of the ADC scan (include/knnx.h:
        knnx_ivfpq_set_threshold_scan): with it on, an IVF-PQ index serves k > 64 (up to 131 072) and range_search; off -- the
        default -- it refuses both as it always has.  False on an index that is not IVF-PQ; setting it there is an error.""")

    def pq_threshold_stats(self):
        """(queries served with k > 64, threshold-scan launches, scans summed over the queries that took part, hits fetched) since the
        index was created (include/knnx.h: knnx_ivfpq_threshold_stats)."""
        return _threshold_stats(self, "ivfpq")

    def pq_arena_bytes(self):
        """(bytes of the code arena, bytes of the row arena -- 0 without a refine store) of an IVF-PQ index."""
        a, b = C.c_int64(0), C.c_int64(0)
        check(self._lib, self._lib.knnx_ivfpq_arena_bytes(self._h, C.byref(a), C.byref(b)), "knnx")
        return int(a.value), int(b.value)

    def pq_codes(self):
        """(codes u8 [ntotal, M], lists int32 [ntotal]) in id order: row i belongs to id id_base + i."""
        n, M = self.ntotal, self.pq_m
        ids = np.empty(n, dtype=np.int64)
        lists = np.empty(n, dtype=np.int32)
        codes = np.empty((n, M), dtype=np.uint8)
        check(self._lib, self._lib.knnx_ivfpq_get_codes(self._h, ids.ctypes.data, lists.ctypes.data, codes.ctypes.data), "knnx")
        order = np.argsort(ids, kind="stable")
        return np.ascontiguousarray(codes[order]), np.ascontiguousarray(lists[order])

    # ------------------------------------------------------------------ IVF-SQ8
    def set_sq_quantizer(self, vmin, vdiff):
        """Make this EMPTY index an IVF-SQ8 one (faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_8bit), not residual):
        vmin, vdiff f32 [d] (train_sq_ranges), one code byte per dimension.  The rows then go in through knnx_ivf_begin / add_assigned
        / end (build_ivfsq_index*), which encode them (include/knnx.h: "IVF-SQ8").  Padding columns get vmin = vdiff = 0."""
        vmin = np.asarray(vmin, dtype=np.float32).reshape(-1)
        vdiff = np.asarray(vdiff, dtype=np.float32).reshape(-1)
        if vmin.shape != (self.d,) or vdiff.shape != (self.d,):
            raise AssertionError(f"vmin and vdiff must be [{self.d}], got {vmin.shape} and {vdiff.shape}")
        a, b = np.zeros(self._dpad, dtype=np.float32), np.zeros(self._dpad, dtype=np.float32)
        a[: self.d], b[: self.d] = vmin, vdiff
        check(self._lib, self._lib.knnx_ivfsq_set_quantizer(self._h, a.ctypes.data, b.ctypes.data), "knnx")

    @property
    def is_sq(self):
        """True on an IVF-SQ8 index."""
        return bool(self._lib.knnx_ivfsq(self._h)) if self._h else False

    def sq_quantizer(self):
        """(vmin, vdiff) f32 [d] as they were given."""
        a, b = np.empty(self._dpad, dtype=np.float32), np.empty(self._dpad, dtype=np.float32)
        check(self._lib, self._lib.knnx_ivfsq_get_quantizer(self._h, a.ctypes.data, b.ctypes.data), "knnx")
        return np.ascontiguousarray(a[: self.d]), np.ascontiguousarray(b[: self.d])

    def sq_codes(self):
        """(codes u8 [ntotal, d], lists int32 [ntotal]) in id order: row i belongs to id id_base + i."""
        n = self.ntotal
        ids = np.empty(n, dtype=np.int64)
        lists = np.empty(n, dtype=np.int32)
        codes = np.empty((n, self._dpad), dtype=np.uint8)
        check(self._lib, self._lib.knnx_ivfsq_get_codes(self._h, ids.ctypes.data, lists.ctypes.data, codes.ctypes.data), "knnx")
        order = np.argsort(ids, kind="stable")
        return np.ascontiguousarray(codes[order][:, : self.d]), np.ascontiguousarray(lists[order])

    sq_threshold_scan = _threshold_scan_property("ivfsq", _own_handle, """The threshold mode of the code scan (include/knnx.h:
        knnx_ivfsq_set_threshold_scan): with it on, an IVF-SQ8 index serves k > 64 (up to 131 072) and range_search; off -- the
        default -- it refuses both as it always has.  False on an index that is not IVF-SQ8; setting it there is an error.""")

    def sq_threshold_stats(self):
        """(queries served with k > 64, threshold-scan launches, launches summed over the queries that took part, hits fetched) since
        the index was created (include/knnx.h: knnx_ivfsq_threshold_stats)."""
        return _threshold_stats(self, "ivfsq")

    # ------------------------------------------------------------------ list-ordered ids (reorder_metadata_by_ivf_index)
    def ivf_old_to_new(self):
        """int64 [ntotal]: old_to_new[i] = id_base + the list-ordered ordinal of the row with id id_base + i (include/knnx.h,
        "List-ordered ids"); with id_base = 0 the array of the reference's get_old_to_new_mapping (ivf_metadata_ordering.py:46-64)."""
        out = np.empty(self.ntotal, dtype=np.int64)
        check(self._lib, self._lib.knnx_ivf_id_order(self._h, out.ctypes.data, None), "knnx")
        return out

    def ivf_new_to_old(self):
        """int64 [ntotal]: the ids of the lists one after the other, list 0 first -- row o of a list-ordered metadata store is the
        source row new_to_old[o] - id_base."""
        out = np.empty(self.ntotal, dtype=np.int64)
        check(self._lib, self._lib.knnx_ivf_id_order(self._h, None, out.ctypes.data), "knnx")
        return out

    def map_ids(self, ids):
        """Result ids (any shape, int64) -> their list-ordered ids, -1 kept: np.take(ivf_old_to_new(), ids - id_base) without the
        table, by a gather kernel over the layout the index holds.  Safe to call from request threads while others search."""
        return _map_ids_call(self._lib, self._lib.knnx_ivf_map_ids, self._h, ids)

    # ------------------------------------------------------------------ growing a built IVF index (include/knnx.h)
    def _grown(self, n_before, lists):
        """After rows were appended: the ids they got; ivf_lists / ivf_row_range follow where the index carries them (save_index).
        lists None: they are not known, and an index that carried them no longer does."""
        n = self.ntotal - n_before
        rng = getattr(self, "ivf_row_range", None)
        base = rng[0] if rng is not None else self._id_base
        if rng is not None:
            self.ivf_row_range = (rng[0], rng[1] + n)
        if getattr(self, "ivf_lists", None) is not None:
            if lists is None:
                del self.ivf_lists
            else:
                self.ivf_lists = np.concatenate([np.asarray(self.ivf_lists, dtype=np.int32), np.asarray(lists, dtype=np.int32)])
        return np.arange(base + n_before, base + n_before + n, dtype=np.int64)

    def ivf_append(self, x, lists=None, chunk=1 << 22):
        """faiss index.add on a BUILT IVF index of any kind (add() keeps refusing it): float16 or float32 rows [n, d] go behind the rows
        of their lists and get the next ids -> int64 [n], the new ids (id_base + ntotal before + i).  `lists` (int32 [n]) names every
        row's list -- in the quantiser space for an index with a rotation, as at build time; None: the library assigns with the index's
        own centroids (what IvfBuilder.assign answers).  The result is bit for bit the index a fresh build over all rows gives.  Every
        call moves the arena once (peak memory: old + new arena), so rows are best appended in large batches; inputs above `chunk` rows
        are converted and appended `chunk` rows at a time.  Concurrent searches see the index before or after a call.  A list-ordered
        metadata store (ivf_old_to_new) must be exported again afterwards."""
        x = np.asarray(x)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"ivf_append expects [n, {self.d}], got {x.shape}")
        if x.dtype not in (np.float16, np.float32):
            raise TypeError(f"ivf_append expects float32 or float16 rows, got {x.dtype}")
        if lists is not None:
            lists = np.ascontiguousarray(lists, dtype=np.int32).reshape(-1)
            if lists.shape[0] != x.shape[0]:
                raise ValueError(f"lists must name one list per row: {lists.shape[0]} for {x.shape[0]} rows")
        n_before, got = self.ntotal, []
        for o in range(0, x.shape[0], int(chunk)):
            rows = np.ascontiguousarray(self._pad(np.asarray(x[o:o + chunk], dtype=np.float16)))
            if lists is not None:
                ls = np.ascontiguousarray(lists[o:o + chunk])
                check(self._lib, self._lib.knnx_ivf_append_assigned(self._h, rows.ctypes.data, rows.shape[0], ls.ctypes.data), "knnx")
            else:
                ls = np.empty(rows.shape[0], dtype=np.int32)
                check(self._lib, self._lib.knnx_ivf_append(self._h, rows.ctypes.data, rows.shape[0], ls.ctypes.data), "knnx")
            got.append(ls)
        if x.shape[0] == 0:  # (still refused on an index that cannot grow)
            check(self._lib, self._lib.knnx_ivf_append(self._h, None, 0, None), "knnx")
        return self._grown(n_before, np.concatenate(got) if got else np.zeros(0, np.int32))

    def ivf_append_device(self, ptr, n):
        """ivf_append for n fp16 rows [n, d] already in HBM on the index's device (a torch tensor's data_ptr(); d % 256 == 0): the
        library assigns them, the rows never visit the host -> the new ids."""
        if self._dpad != self.d:
            raise HipLibraryError("device rows must already be padded to a multiple of 256 columns")
        n_before = self.ntotal
        ls = np.empty(int(n), dtype=np.int32)
        check(self._lib, self._lib.knnx_ivf_append_device(self._h, C.c_void_p(int(ptr)), int(n), ls.ctypes.data), "knnx")
        return self._grown(n_before, ls)

    def merge_from(self, other):
        """faiss merge_from / merge_ondisk (clip_back_prepro/index_combiner.py): every row of `other`, a built IVF index of the same
        kind with bit-equal centroids and quantiser, goes into this one -> the new ids; other's id j becomes id_base + ntotal before +
        (j - other's id_base).  Codes and rows are copied through host memory, never encoded again, so `other` may live on another
        device.  Unlike faiss, `other` is left untouched (close it when it is no longer needed)."""
        if not isinstance(other, Mi355xIndex):
            raise TypeError("merge_from takes a Mi355xIndex")
        n_before = self.ntotal
        check(self._lib, self._lib.knnx_ivf_merge_from(self._h, other._h), "knnx")  # pylint: disable=protected-access
        lists = getattr(other, "ivf_lists", None)
        if lists is None and other.pq_m:
            lists = other.pq_codes()[1]
        elif lists is None and other.is_sq:
            lists = other.sq_codes()[1]
        for name in ("ivf_source", "embeddings_folder", "ivf_folder", "ivf_folder_files"):  # the rows no longer come from one folder
            if hasattr(self, name):
                delattr(self, name)
        return self._grown(n_before, lists)

    # ------------------------------------------------------------------ shrinking a built IVF index (include/knnx.h)
    def _shrunk(self, kept, base):
        """After rows were removed (kept: the old ids of the survivors in new-id order): ivf_lists / ivf_row_range follow where the index
        carries them, and what bound the index to the folder it was built from is dropped -- the folder's rows no longer are its rows."""
        if getattr(self, "ivf_lists", None) is not None:
            self.ivf_lists = np.ascontiguousarray(np.asarray(self.ivf_lists, dtype=np.int32)[kept - base])
        if getattr(self, "ivf_row_range", None) is not None:
            self.ivf_row_range = (self.ivf_row_range[0], self.ivf_row_range[0] + len(kept))
        for name in ("ivf_source", "embeddings_folder", "ivf_folder", "ivf_folder_files"):
            if hasattr(self, name):
                delattr(self, name)

    def ivf_remove(self, ids):
        """Remove rows from a BUILT IVF index of any kind: `ids` (integers, any shape) names them; entries that name no row (-1, outside
        [id_base, id_base + ntotal)) are ignored and duplicates count once.  Ids are positional, so the survivors are RENUMBERED densely
        in id order, as faiss' IndexFlat.remove_ids does -> kept, int64 [ntotal after]: the OLD ids of the survivors in new-id order --
        new id id_base + i was old id kept[i].  The caller filters its embeddings and its metadata store with kept - id_base.  The
        result is bit for bit the index a fresh build over the surviving rows gives; concurrent searches see the index before or after
        the call; peak memory is old + new arena.  A list-ordered metadata store (ivf_old_to_new) must be exported again afterwards.
        The index no longer belongs to the folder it was built from: save_index of an IVF-Flat or refine index then needs
        embeddings_folder= naming a folder that holds the surviving rows.  A sharded index has no removal (the shards' row ranges would
        shift), and an index handed to ShardedMi355xIndex must not be shrunk afterwards."""
        ids = np.asarray(ids)
        if ids.dtype.kind not in "iu":
            raise TypeError(f"ivf_remove expects integer ids, got {ids.dtype}")
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        n_before = self.ntotal
        rng = getattr(self, "ivf_row_range", None)
        base = rng[0] if rng is not None else self._id_base
        removed = C.c_int64(0)
        # (an empty array still goes to the library: an index that cannot shrink refuses)
        check(self._lib, self._lib.knnx_ivf_remove_ids(self._h, ids.ctypes.data if ids.size else None, int(ids.size), C.byref(removed)), "knnx")
        alive = np.ones(n_before, dtype=bool)
        o = ids - base
        alive[o[(o >= 0) & (o < n_before)]] = False
        kept = base + np.flatnonzero(alive).astype(np.int64)
        if n_before - len(kept) != removed.value or len(kept) != self.ntotal:
            raise HipLibraryError(f"ivf_remove: the library removed {removed.value} rows and holds {self.ntotal}, the ids name {n_before - len(kept)} of {n_before}")
        if removed.value:
            self._shrunk(kept, base)
        return kept

    def remove_ids(self, ids):
        """faiss Index.remove_ids: ivf_remove(ids) -> the number of rows removed.  Mind that the survivors are renumbered (ivf_remove)."""
        n_before = self.ntotal
        return n_before - len(self.ivf_remove(ids))

    def ivf_remove_stats(self):
        """What the most recent removal spent (include/knnx.h: knnx_ivf_remove_stats): dict of mark_ms, plan_ms, move_ms, ids_ms,
        moved_bytes, n_removed."""
        ms = [C.c_double() for _ in range(4)]
        mb, nr = C.c_int64(), C.c_int64()
        check(self._lib, self._lib.knnx_ivf_remove_stats(self._h, *[C.byref(m) for m in ms], C.byref(mb), C.byref(nr)), "knnx")
        return dict(mark_ms=ms[0].value, plan_ms=ms[1].value, move_ms=ms[2].value, ids_ms=ms[3].value, moved_bytes=mb.value, n_removed=nr.value)

    # ------------------------------------------------------------------ searching
    def _search_raw(self, q, k, want_r):
        n = q.shape[0]
        qp = np.ascontiguousarray(self._pad(q))
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        R = np.empty((n, k, self._dpad), dtype=np.float32) if want_r else None
        check(self._lib, self._lib.knnx_search(self._h, qp.ctypes.data, n, int(k), D.ctypes.data, I.ctypes.data,
                                               R.ctypes.data if want_r else None), "knnx")
        if want_r and self._dpad != self.d:
            R = np.ascontiguousarray(R[:, :, : self.d])
        return D, I, R

    def reconstruct_batch(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        out = np.empty((keys.shape[0], self._dpad), dtype=np.float32)
        check(self._lib, self._lib.knnx_reconstruct(self._h, keys.ctypes.data, keys.shape[0], out.ctypes.data), "knnx")
        return np.ascontiguousarray(out[:, : self.d])

    DEDUP_PAIR_CAP = 512

    def search_dedup(self, x, k, threshold=0.94, want_r=False):
        """One request of KnnService.knn_search with its dedup fused (knnx.h: knnx_search_dedup; clip_back.py:362 + :290-309):
        x float32 [1, d], k <= 64 -> (D [1, k], I [1, k], R [1, k, d] or None, links int32 [n_links, 2] of result ranks i < j
        whose normalised stored vectors have inner product > threshold, or None when there were more links than the device
        keeps -- take the general path then).  Concurrent callers share one scan, one gather and one link launch."""
        q = np.ascontiguousarray(self._pad(_as_queries(x, self.d)))
        if q.shape[0] != 1 or not 0 < k <= 64:
            raise AssertionError("search_dedup serves one query and k <= 64")
        k = int(k)
        D = np.empty((1, k), dtype=np.float32)
        I = np.empty((1, k), dtype=np.int64)
        R = np.empty((1, k, self._dpad), dtype=np.float32) if want_r else None
        pairs = np.empty((self.DEDUP_PAIR_CAP, 2), dtype=np.int32)
        n = C.c_int(0)
        check(self._lib, self._lib.knnx_search_dedup(self._h, q.ctypes.data, k, D.ctypes.data, I.ctypes.data, R.ctypes.data if want_r else None,
                                                     C.c_float(threshold), pairs.ctypes.data, self.DEDUP_PAIR_CAP, C.byref(n)), "knnx")
        if want_r and self._dpad != self.d:
            R = np.ascontiguousarray(R[:, :, : self.d])
        return D, I, R, (pairs[: n.value].copy() if n.value <= self.DEDUP_PAIR_CAP else None)

    FILTER_MAX_K = 8192
    DROP_DUPLICATE, DROP_VIOLENT, DROP_UNSAFE = 1, 2, 4

    def search_filtered(self, x, k, dedup_thr=None, violence=None, safety=None, safety_thr=0.5):
        """One request of KnnService.knn_search with its whole post filter on the device (knnx.h: knnx_search_filtered;
        clip_back.py:343-399): x float32 [1, d], k <= 8192 -> (D [1, k], I [1, k], drop uint8 [k], stats).  D, I are what search(x, k)
        returns; drop[i] carries DROP_DUPLICATE (rank i is not the best-ranked member of its group of near-duplicates: normalised stored
        rows with inner product > dedup_thr, transitively; None: no dedup), DROP_VIOLENT (`violence`: a bias-free one-layer device head
        [P, d] over the prompt embeddings; the best-matching prompt is prompt 1) and DROP_UNSAFE (`safety`: a device head whose output 0
        is > safety_thr).  The heads are objects with `._h` (a knnx_mlp handle) on this index's device, e.g. service.Mi355xSafetyHead.
        stats: dict(n_valid, n_links, links_overflowed, cc_rounds); with links_overflowed the request had more than 2^20 links, NO
        duplicate bit is set and dedup is the caller's (reconstruct_batch + a range search).  Only D, I and the k bytes travel."""
        q = np.ascontiguousarray(self._pad(_as_queries(x, self.d)))
        if q.shape[0] != 1:
            raise AssertionError("search_filtered serves one query")
        k = int(k)
        D = np.empty((1, max(k, 1)), dtype=np.float32)
        I = np.empty((1, max(k, 1)), dtype=np.int64)
        drop = np.zeros(max(k, 1), dtype=np.uint8)
        stats = (C.c_int32 * 4)()
        check(self._lib, self._lib.knnx_search_filtered(
            self._h, q.ctypes.data, k, self.d, 0 if dedup_thr is None else 1, C.c_float(0.0 if dedup_thr is None else dedup_thr),
            violence._h if violence is not None else None, safety._h if safety is not None else None,  # pylint: disable=protected-access
            C.c_float(safety_thr), D.ctypes.data, I.ctypes.data, drop.ctypes.data, C.cast(stats, C.c_void_p)), "knnx")
        return D, I, drop, dict(n_valid=int(stats[0]), n_links=int(stats[1]), links_overflowed=int(stats[2]), cc_rounds=int(stats[3]))

    def i8_served(self):
        """Queries answered through the int8 first stage of the flat scans (include/knnx.h: knnx_i8_served); results are exact
        either way."""
        return int(self._lib.knnx_i8_served(self._h))

    def i8_rows(self):
        """Rows the int8 copy holds at the moment (include/knnx.h: knnx_i8_rows): ntotal, fewer for a partial copy, 0 for none."""
        return int(self._lib.knnx_i8_rows(self._h))

    def i8_planes(self):
        """0: no int8 copy at the moment; 1 / 2: int8 planes per query of the first stage (include/knnx.h: knnx_i8_planes)."""
        return int(self._lib.knnx_i8_planes(self._h))

    def i8_dominant(self):
        """Columns the int8 first stage treats as dominant (include/knnx.h: knnx_i8_dominant): a list of 0 .. 4 column numbers."""
        cols = (C.c_int * 4)()
        n = int(self._lib.knnx_i8_dominant(self._h, cols))
        return [int(cols[j]) for j in range(max(n, 0))]

    def coalesce_stats(self):
        """(batches served, queries in them, largest batch) of the library's request coalescer."""
        b, q, m = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(self._lib, self._lib.knnx_coalesce_stats(self._h, C.byref(b), C.byref(q), C.byref(m)), "knnx")
        return int(b.value), int(q.value), int(m.value)

    def range_search(self, x, thresh):
        q = np.ascontiguousarray(self._pad(_as_queries(x, self.d)))
        n = q.shape[0]
        lims = np.zeros(n + 1, dtype=np.int64)
        # one pass when the hits fit a guessed capacity (the per-request dedup finds ~n hits for n vectors); the two-call
        # protocol (count, then fill) otherwise
        guess = max(4096, 16 * n)
        D = np.empty(guess, dtype=np.float32)
        I = np.empty(guess, dtype=np.int64)
        rc = self._lib.knnx_range_search_once(self._h, q.ctypes.data, n, C.c_float(thresh), lims.ctypes.data, D.ctypes.data, I.ctypes.data, guess)
        if rc == 0:
            total = int(lims[n])
            return lims, D[:total].copy(), I[:total].copy()
        if rc < 0:
            check(self._lib, rc, "knnx")
        total = int(lims[n])
        D = np.empty(total, dtype=np.float32)
        I = np.empty(total, dtype=np.int64)
        if total:
            check(self._lib, self._lib.knnx_range_search(self._h, q.ctypes.data, n, C.c_float(thresh), lims.ctypes.data,
                                                         D.ctypes.data, I.ctypes.data), "knnx")
        return lims, D, I

    # ------------------------------------------------------------------ device-buffer path (bench, sharded search)
    def search_device(self, q_ptr, n, k, D_ptr, I_ptr, stream=None):
        check(self._lib, self._lib.knnx_search_device(self._h, C.c_void_p(int(q_ptr)), int(n), int(k), C.c_void_p(int(D_ptr)),
                                                      C.c_void_p(int(I_ptr)), C.c_void_p(int(stream)) if stream else None), "knnx")

    def profile(self, on):
        check(self._lib, self._lib.knnx_profile_enable(self._h, 1 if on else 0), "knnx")

    def stats(self):
        """(queries served by a proof-based scan, queries whose exactness proof failed and were re-run exactly)."""
        a, b = C.c_int64(0), C.c_int64(0)
        check(self._lib, self._lib.knnx_get_stats(self._h, C.byref(a), C.byref(b)), "knnx")
        return int(a.value), int(b.value)

    def profile_get(self):
        n, ms = C.c_int64(0), C.c_double(0.0)
        check(self._lib, self._lib.knnx_profile_get(self._h, C.byref(n), C.byref(ms)), "knnx")
        return int(n.value), float(ms.value)


class ShardedMi355xIndex(_FaissShaped):
    """Row-sharded index over several GPUs of ONE process behind the same faiss-shaped surface -- the object that goes
    into `ClipResource.image_index` (clip_back.py:781-782) when the index needs more than one GPU (BASELINE config 5).
    Shard g = rows [g*T/G, (g+1)*T/G) on devices[g]; ids = global row numbers.  C ABI: knnx_shards_* (include/knnx.h)."""

    def __init__(self, d, devices, coalesce=True, _adopt=None):
        self._lib = load_library()
        self.d = int(d)
        self._dpad = (self.d + 255) // 256 * 256
        self.devices = [int(x) for x in devices]
        h = C.c_void_p()
        dv = (C.c_int * len(self.devices))(*self.devices)
        if _adopt is None:
            check(self._lib, self._lib.knnx_shards_create(len(self.devices), dv, self._dpad, METRIC_INNER_PRODUCT, C.byref(h)), "knnx")
        else:
            shards, row_lo = _adopt
            hs = (C.c_void_p * len(shards))(*[sh._h for sh in shards])  # pylint: disable=protected-access
            lo = (C.c_int64 * len(shards))(*[int(x) for x in row_lo])
            check(self._lib, self._lib.knnx_shards_adopt(len(shards), hs, dv, lo, C.byref(h)), "knnx")
            for sh in shards:
                sh._h = None  # pylint: disable=protected-access  (owned by the sharded handle now)
        self._h = h
        self.metric_type = METRIC_INNER_PRODUCT
        self.is_trained = True
        self._init_queue(coalesce)

    @classmethod
    def from_shards(cls, shards, row_lo, coalesce=True):
        """Adopt per-device `Mi355xIndex` objects (flat, IVF-Flat or IVF-PQ -- all with the same rotation or none; shard g built with
        id_base = row_lo[g])."""
        return cls(shards[0].d, [sh.device for sh in shards], coalesce=coalesce, _adopt=(shards, row_lo))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.knnx_shards_destroy(h)

    @property
    def ntotal(self):
        return int(self._lib.knnx_shards_ntotal(self._h))

    @property
    def nlist(self):
        """Lists of the (shared) coarse quantiser when the shards are IVF-Flat, else 0."""
        return int(self._lib.knnx_ivf_nlist(C.c_void_p(self._lib.knnx_shards_get(self._h, 0)))) if self.nshards else 0

    @property
    def nprobe(self):
        """What the shards carry (knnx_ivf_nprobe of the first IVF shard): an index adopted with from_shards() keeps the value its
        shards were built with (the wrapper used to answer 1 until it had been set, and knn_search's wide path then
        'restored' 1 on every shard)."""
        for g in range(self.nshards):
            sh = C.c_void_p(self._lib.knnx_shards_get(self._h, g))
            if self._lib.knnx_ivf_nlist(sh) > 0:
                return int(self._lib.knnx_ivf_nprobe(sh))
        return getattr(self, "_nprobe", 1)

    @nprobe.setter
    def nprobe(self, v):
        """IVF-Flat shards: faiss `extract_index_ivf(index).nprobe = v` on every shard (clip_back.py:357-369)."""
        for g in range(self.nshards):
            sh = C.c_void_p(self._lib.knnx_shards_get(self._h, g))
            if self._lib.knnx_ivf_nlist(sh) > 0:
                check(self._lib, self._lib.knnx_ivf_set_nprobe(sh, int(v)), "knnx")
        self._nprobe = int(v)

    @property
    def pq_refine(self):
        """True when the shards are IVF-PQ indexes with a refine store (all of them or none: knnx_shards_adopt)."""
        return bool(self._lib.knnx_ivfpq_refine(C.c_void_p(self._lib.knnx_shards_get(self._h, 0)))) if self.nshards else False

    @property
    def k_factor(self):
        """Candidates per result of a refine search, as carried by the first shard (Mi355xIndex.k_factor)."""
        return int(self._lib.knnx_ivfpq_k_factor(C.c_void_p(self._lib.knnx_shards_get(self._h, 0)))) if self.nshards else 1

    @k_factor.setter
    def k_factor(self, v):
        for g in range(self.nshards):
            check(self._lib, self._lib.knnx_ivfpq_set_k_factor(C.c_void_p(self._lib.knnx_shards_get(self._h, g)), int(v)), "knnx")

    pq_threshold_scan = _threshold_scan_property("ivfpq", _shard_handles, """The threshold-scan switch as carried by the first shard
        (Mi355xIndex.pq_threshold_scan); the setter sets every shard.""")
    sq_threshold_scan = _threshold_scan_property("ivfsq", _shard_handles, """The IVF-SQ8 threshold-scan switch as carried by the first
        shard (Mi355xIndex.sq_threshold_scan); the setter sets every shard.""")

    @property
    def nshards(self):
        return int(self._lib.knnx_shards_count(self._h))

    @property
    def exchange(self):
        """'rccl' (one grouped ncclAllGather of the per-shard top-k lists) or 'peer-copies' (include/knnx.h: knnx_shards_exchange)."""
        return "rccl" if int(self._lib.knnx_shards_exchange(self._h)) == 1 else "peer-copies"

    def reserve(self, total_rows):
        """Fix the row range of every shard; must precede add()."""
        check(self._lib, self._lib.knnx_shards_reserve(self._h, int(total_rows)), "knnx")

    def add(self, x):
        x = np.asarray(x)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise AssertionError(f"add expects [n, {self.d}], got {x.shape}")
        if x.dtype == np.float16:
            x = np.ascontiguousarray(self._pad(x))
            check(self._lib, self._lib.knnx_shards_add_f16(self._h, x.ctypes.data, x.shape[0]), "knnx")
        elif x.dtype == np.float32:
            x = np.ascontiguousarray(self._pad(x))
            check(self._lib, self._lib.knnx_shards_add_f32(self._h, x.ctypes.data, x.shape[0]), "knnx")
        else:
            raise TypeError(f"add expects float32 or float16 rows, got {x.dtype}")

    def synth_fill(self, rows_per_shard, seed):
        if self._dpad != self.d:
            raise HipLibraryError("synthetic fill needs d % 256 == 0")
        check(self._lib, self._lib.knnx_shards_synth_fill(self._h, int(rows_per_shard), C.c_uint64(int(seed))), "knnx")

    def _search_raw(self, q, k, want_r):
        n = q.shape[0]
        qp = np.ascontiguousarray(self._pad(q))
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        R = np.empty((n, k, self._dpad), dtype=np.float32) if want_r else None
        check(self._lib, self._lib.knnx_shards_search(self._h, qp.ctypes.data, n, int(k), D.ctypes.data, I.ctypes.data,
                                                      R.ctypes.data if want_r else None), "knnx")
        if want_r and self._dpad != self.d:
            R = np.ascontiguousarray(R[:, :, : self.d])
        return D, I, R

    def reconstruct_batch(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        out = np.empty((keys.shape[0], self._dpad), dtype=np.float32)
        check(self._lib, self._lib.knnx_shards_reconstruct(self._h, keys.ctypes.data, keys.shape[0], out.ctypes.data), "knnx")
        return np.ascontiguousarray(out[:, : self.d])

    def range_search(self, x, thresh):
        q = np.ascontiguousarray(self._pad(_as_queries(x, self.d)))
        n = q.shape[0]
        lims = np.zeros(n + 1, dtype=np.int64)
        check(self._lib, self._lib.knnx_shards_range_search(self._h, q.ctypes.data, n, C.c_float(thresh), lims.ctypes.data, None, None), "knnx")
        total = int(lims[n])
        D = np.empty(total, dtype=np.float32)
        I = np.empty(total, dtype=np.int64)
        if total:
            check(self._lib, self._lib.knnx_shards_range_search(self._h, q.ctypes.data, n, C.c_float(thresh), lims.ctypes.data,
                                                                D.ctypes.data, I.ctypes.data), "knnx")
        return lims, D, I

    def ivf_old_to_new(self):
        """int64 [ntotal]: the concatenation of the shards' old_to_new arrays (each list-sorted inside its own row range): a
        permutation of [0, ntotal) (Mi355xIndex.ivf_old_to_new)."""
        out = np.empty(self.ntotal, dtype=np.int64)
        check(self._lib, self._lib.knnx_shards_id_order(self._h, out.ctypes.data, None), "knnx")
        return out

    def ivf_new_to_old(self):
        """int64 [ntotal]: the concatenation of the shards' new_to_old arrays (Mi355xIndex.ivf_new_to_old)."""
        out = np.empty(self.ntotal, dtype=np.int64)
        check(self._lib, self._lib.knnx_shards_id_order(self._h, None, out.ctypes.data), "knnx")
        return out

    def map_ids(self, ids):
        """Result ids (any shape, int64) -> their list-ordered ids, -1 kept; every id is translated by the shard that owns it."""
        return _map_ids_call(self._lib, self._lib.knnx_shards_map_ids, self._h, ids)

    def shard_stats(self):
        """Per-shard (proof-served queries, proof failures)."""
        out = []
        for g in range(self.nshards):
            a, b = C.c_int64(0), C.c_int64(0)
            check(self._lib, self._lib.knnx_get_stats(C.c_void_p(self._lib.knnx_shards_get(self._h, g)), C.byref(a), C.byref(b)), "knnx")
            out.append((int(a.value), int(b.value)))
        return out


def get_old_to_new_mapping(index):
    """The reference's get_old_to_new_mapping(index) (ivf_metadata_ordering.py:46-64) for an IVF index of this package: int64
    [ntotal], entry i = the position of id i in a metadata store ordered by inverted list.  One pass over the id map on the device
    instead of a Python loop over the lists."""
    return index.ivf_old_to_new()


def search_to_new_ids(index, query, k):
    """The reference's search_to_new_ids(index, query, k) (ivf_metadata_ordering.py:17-43): (distances [n, k], the list-ordered ids
    of the FIRST query's results [k], -1 kept).  The search is the plain search; only its ids are translated (Mi355xIndex.map_ids)."""
    distances, indices = index.search(query, k)
    return distances, index.map_ids(indices[0])


def embedding_files(folder):
    """The `img_emb_*.npy` / `text_emb_*.npy` files of one `clip inference` output folder, in partition
    order (zero-padded names sort correctly: writer.py:22,67)."""
    # (not the sidecars save_index() writes -- ivf_centroids.npy / ivf_lists.npy: an index saved INTO its embeddings folder must not
    # turn into two more partitions at the next load)
    files = sorted(f for f in glob.glob(os.path.join(folder, "*.npy")) if not os.path.basename(f).startswith("ivf_"))
    if not files:
        raise ValueError(f"no .npy embedding files under {folder}")
    return files


def load_index(path, device=0, row_range=None, enable_faiss_memory_mapping=False, devices=None, embeddings_folder=None):  # pylint: disable=unused-argument
    """Build an HBM-resident flat index from a folder of fp16 `.npy` partitions -- or, when `path` is a folder written by
    `save_index()` (it holds ivf_manifest.json), re-create that IVF-Flat index without training or assigning anything; a folder
    with ivf_pq_manifest.json / ivf_sq_manifest.json is read as that IVF-PQ / IVF-SQ8 index, straight from its saved codes.

    Takes the place of clip_back.py:589-596 (`faiss.read_index`) for this index type; ids are the global
    row order of the concatenated partitions = the metadata row order (clip_back.py:401-417).
    `row_range=(lo, hi)` loads one shard of a row-sharded index and sets its id base to `lo` (one process per GPU);
    `devices=[0, 1, ...]` builds ONE object that row-shards the whole folder over those GPUs of this process
    (`ShardedMi355xIndex`, the KnnService case).  `enable_faiss_memory_mapping` is accepted for call compatibility:
    rows are always resident in HBM; the files themselves are read through np.load(mmap_mode="r").
    """
    if os.path.isfile(os.path.join(path, IVFPQ_MANIFEST)):  # a saved IVF-PQ index: self-contained unless it has a refine store
        return _load_ivfpq_index(path, device=device, row_range=row_range, devices=devices, embeddings_folder=embeddings_folder)
    if os.path.isfile(os.path.join(path, IVFSQ_MANIFEST)):  # a saved IVF-SQ8 index: self-contained (codes, not rows)
        return _load_ivfsq_index(path, device=device, row_range=row_range, devices=devices)
    if os.path.isfile(os.path.join(path, IVF_MANIFEST)):  # a built IVF-Flat index saved by save_index(): no k-means, no assignment
        return _load_ivf_index(path, device=device, row_range=row_range, devices=devices)
    src = FolderRows(path)
    files, shapes, d, total = src.files, src.shapes, src.d, src.n
    lo, hi = (0, total) if row_range is None else row_range
    if devices is not None:
        if row_range is not None:
            raise ValueError("row_range and devices are mutually exclusive")
        index = ShardedMi355xIndex(d, devices)
        index.reserve(total)
    else:
        index = Mi355xIndex(d, device=device, id_base=lo)
        index.reserve(max(hi - lo, 0))
    start = 0
    for f, s in zip(files, shapes):
        a0, a1 = max(lo, start), min(hi, start + s[0])
        if a1 > a0:
            a = np.load(f, mmap_mode="r")[a0 - start:a1 - start]
            index.add(np.ascontiguousarray(a) if a.dtype in (np.float16, np.float32) else np.asarray(a, dtype=np.float32))
        start += s[0]
    return index


# ------------------------------------------------------------------------------------------------------------
# IVF-Flat index build (BASELINE config 5; takes the place of the autofaiss call of clip_index.py:12-66 for this
# index type).  The arithmetic runs on the GPU through the builder entry points of include/knnx.h: list assignment is
# the MFMA assignment kernel (csrc/knn_rq_kernels.hip: knn_assign_kernel), the Lloyd update one workgroup per list, the
# final layout a scatter kernel; the host keeps integer bookkeeping only (bincount, prefix sums, stable ranks).
# ------------------------------------------------------------------------------------------------------------
class IvfBuilder:
    """Centroids (and optionally a training sample) resident on one GPU: knnx_ivfb_* of include/knnx.h."""

    def __init__(self, d, nlist, device=0):
        self._lib = load_library()
        self.d, self.nlist, self.device = int(d), int(nlist), int(device)
        self._dpad = (self.d + 255) // 256 * 256
        h = C.c_void_p()
        check(self._lib, self._lib.knnx_ivfb_create(self.device, self._dpad, self.nlist, C.byref(h)), "knnx")
        self._h = h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.knnx_ivfb_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass

    def _rows(self, x):
        x = np.asarray(x)
        if x.dtype != np.float16:
            x = x.astype(np.float16)
        if self._dpad != self.d:
            out = np.zeros((x.shape[0], self._dpad), dtype=np.float16)
            out[:, : self.d] = x
            x = out
        return np.ascontiguousarray(x)

    def set_centroids(self, c):
        c = self._rows(c)
        assert c.shape[0] == self.nlist
        check(self._lib, self._lib.knnx_ivfb_set_centroids(self._h, c.ctypes.data), "knnx")

    def centroids(self):
        out = np.empty((self.nlist, self._dpad), dtype=np.float16)
        check(self._lib, self._lib.knnx_ivfb_get_centroids(self._h, out.ctypes.data), "knnx")
        return np.ascontiguousarray(out[:, : self.d])

    def set_sample(self, x):
        x = self._rows(x)
        self._n_sample = x.shape[0]
        check(self._lib, self._lib.knnx_ivfb_set_sample(self._h, x.ctypes.data, x.shape[0]), "knnx")

    def assign_sample(self):
        out = np.empty(self._n_sample, dtype=np.int32)
        check(self._lib, self._lib.knnx_ivfb_assign_sample(self._h, out.ctypes.data), "knnx")
        return out

    def update(self, lists):
        """One Lloyd update from the resident sample; returns the list sizes (empty lists keep their centroid)."""
        order = np.ascontiguousarray(np.argsort(lists, kind="stable").astype(np.int64))
        sizes = np.bincount(lists, minlength=self.nlist).astype(np.int64)
        off = np.zeros(self.nlist + 1, dtype=np.int64)
        np.cumsum(sizes, out=off[1:])
        check(self._lib, self._lib.knnx_ivfb_update(self._h, order.ctypes.data, off.ctypes.data), "knnx")
        return sizes

    def assign(self, x):
        """List id (argmax over the centroids, ties -> smaller id) of every row of x; rows are streamed in 1 Mi-row chunks."""
        x = self._rows(x)
        out = np.empty(x.shape[0], dtype=np.int32)
        check(self._lib, self._lib.knnx_ivfb_assign(self._h, x.ctypes.data, x.shape[0], out.ctypes.data), "knnx")
        return out


    # ---- rows that are already in HBM (device pointers; SURVEY 8 row f1 at BASELINE config 5's size) ----
    def set_sample_device(self, dev_ptr, n):
        """Borrow n fp16 rows [n, d_padded] of device memory as the training sample (the caller keeps them alive)."""
        self._n_sample = int(n)
        check(self._lib, self._lib.knnx_ivfb_set_sample_device(self._h, C.c_void_p(dev_ptr), int(n)), "knnx")

    def seed_from_sample(self, list_ids, sample_rows):
        """centroid list_ids[i] := sample row sample_rows[i] (initial seeding / re-seeding of empty lists)."""
        li = np.ascontiguousarray(list_ids, dtype=np.int32)
        sr = np.ascontiguousarray(sample_rows, dtype=np.int64)
        assert li.shape == sr.shape
        check(self._lib, self._lib.knnx_ivfb_seed_from_sample(self._h, li.ctypes.data, sr.ctypes.data, li.size), "knnx")

    def lloyd(self):
        """One Lloyd iteration over the resident sample, driven inside the library; returns the list sizes."""
        sizes = np.empty(self.nlist, dtype=np.int64)
        check(self._lib, self._lib.knnx_ivfb_lloyd(self._h, sizes.ctypes.data), "knnx")
        return sizes

    def assign_device(self, rows_ptr, n, lists_ptr):
        """lists[i] = list of device row i (int32 device array); the list sizes accumulate in the builder."""
        check(self._lib, self._lib.knnx_ivfb_assign_device(self._h, C.c_void_p(rows_ptr), int(n), C.c_void_p(lists_ptr)), "knnx")

    def list_sizes(self, reset=False):
        sizes = np.empty(self.nlist, dtype=np.int64)
        check(self._lib, self._lib.knnx_ivfb_list_sizes(self._h, sizes.ctypes.data, int(bool(reset))), "knnx")
        return sizes


def synth_rows_device(dst_ptr, row_begin, n, d, seed, kind=0, n_clusters=0, row_stride=1, device=0, stream=None):
    """Benchmark corpus rows generated into device memory (knnx_synth_rows_device): kind 0 isotropic, 1 config-5 mixture, 2 isotropic
    with three dominant columns (CLIP-like anisotropy)."""
    lib = load_library()
    check(lib, lib.knnx_synth_rows_device(int(device), C.c_void_p(dst_ptr), int(row_begin), int(row_stride), int(n), int(d),
                                          C.c_uint64(seed), int(kind), int(n_clusters), C.c_void_p(stream) if stream else None), "knnx")


def rebalance_centroids(cent, sizes, rng, small=0.5, big=2.0, eps=0.05):
    """Split-and-merge step of the k-means (what faiss' Clustering does for empty clusters -- `split_clusters` -- extended to the
    small ones): every list with fewer than `small` x the mean size (smallest first, and only while it is under a quarter of the list it
    would split) gives its centroid up, and the currently largest list (above `big` x the mean) is split by replacing its centroid c with the unit vectors of c + delta and c - delta (delta = eps |c| times a
    random sign vector / sqrt(d)): the next Lloyd iteration deals the big list's members between the two halves, the small list's
    few members move to their next-nearest centroids.  Round 5: BASELINE config 5's shard had lists of 1 / 1 880 /
    14 993 rows (min / median / max) and scanned 1.2 - 1.3 x the bytes of the balanced-list model.  Returns the number of splits;
    `cent` (float32 [nlist, d]) is changed in place."""
    import heapq  # pylint: disable=import-outside-toplevel

    sizes = np.asarray(sizes, dtype=np.float64)
    mean = sizes.mean()
    donors = [int(i) for i in np.argsort(sizes) if sizes[i] < small * mean]
    heap = [(-float(sizes[i]), int(i)) for i in np.flatnonzero(sizes > big * mean)]
    heapq.heapify(heap)
    taken = set(donors)
    n = 0
    for i in donors:
        while heap and heap[0][1] in taken:
            heapq.heappop(heap)
        if not heap or -heap[0][0] <= big * mean:
            break
        if sizes[i] > -heap[0][0] / 4:  # giving up a list a quarter the size of the one it would split gains nothing
            break
        s, j = heapq.heappop(heap)
        c = cent[j].astype(np.float64)
        delta = eps * np.linalg.norm(c) / np.sqrt(c.size) * rng.choice((-1.0, 1.0), size=c.size)
        a, b = c + delta, c - delta
        cent[j] = (a / max(np.linalg.norm(a), 1e-30)).astype(cent.dtype)
        cent[i] = (b / max(np.linalg.norm(b), 1e-30)).astype(cent.dtype)
        heapq.heappush(heap, (s / 2, j))  # each half may be split again
        heapq.heappush(heap, (s / 2, i))
        taken.discard(i)
        n += 1
    return n


def train_ivf_centroids_device(builder, sample_ptr, n_sample, niter=8, seed=0, balance=True):
    """k-means over a device-resident sample with `builder` (IvfBuilder): seeds from distinct random sample rows, runs
    `niter` Lloyd iterations, re-seeds empty lists on random sample rows and -- `balance`, all but the last two iterations -- moves the
    centroids of the smallest lists into the largest ones (rebalance_centroids).  Returns the list sizes of the last iteration."""
    rng = np.random.default_rng(seed)
    builder.set_sample_device(sample_ptr, n_sample)
    builder.seed_from_sample(np.arange(builder.nlist), np.sort(rng.choice(n_sample, builder.nlist, replace=False)))
    sizes = None
    for it in range(niter):
        sizes = builder.lloyd()
        if balance and it < niter - 2 and builder.nlist >= 16:
            cent = builder.centroids().astype(np.float32)
            if rebalance_centroids(cent, sizes, rng):
                builder.set_centroids(cent.astype(np.float16))
                continue
        empty = np.flatnonzero(sizes == 0)
        if empty.size:
            builder.seed_from_sample(empty, rng.choice(n_sample, empty.size, replace=False))
    return sizes


def _download_i32(dev_ptr, n, device):  # pylint: disable=unused-argument
    """n int32 from device memory to a numpy array (plain hipMemcpy through the HIP runtime libclipx.so already links)."""
    out = np.empty(int(n), dtype=np.int32)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    rc = hip.hipMemcpy(out.ctypes.data, C.c_void_p(int(dev_ptr)), out.nbytes, 2)  # hipMemcpyDeviceToHost
    if rc != 0:
        raise HipLibraryError(f"hipMemcpy (device -> host) failed with code {rc}")
    return out


def _release_cached_device_memory():
    import sys

    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available():
        torch.cuda.empty_cache()


def build_ivf_index_device(fill_rows, n, d, nlist, nprobe=16, niter=8, seed=0, device=0, id_base=0, sample_rows=None,
                           chunk=1 << 20, alloc=None, points_per_centroid=64, keep_lists=False):
    """IVF-Flat index over n rows that are PRODUCED ON THE GPU (BASELINE config 5: one 125 M x 1024 shard = 256 GB of HBM).

    `fill_rows(dst_ptr, row0, count, stride)` writes fp16 rows row0, row0 + stride, ... ([count, d], d a multiple of 256)
    at device address dst_ptr; it is called for the training sample (stride > 1) and twice per chunk (assignment pass and
    scatter pass) -- the corpus never exists twice.  **fill_rows must have COMPLETED when it returns** (synchronise the stream it
    launched on): the library's assignment / scatter kernels read the buffer on the index's own non-blocking streams right after,
    and nothing orders those behind a producer that is still running on another stream.  `alloc(nbytes)` returns (device pointer, keep-alive object) for the
    scratch buffers (sample, one chunk of rows, 4 bytes per row of list ids); default: torch uint8 tensors (torch is
    this package's device-memory plumbing).  Returns (index, stats dict)."""
    import time

    assert d % 256 == 0, "device builds take padded rows (d % 256 == 0)"
    lib = load_library()
    if alloc is None:
        def alloc(nbytes):
            import torch

            t = torch.empty(int(nbytes), dtype=torch.uint8, device=f"cuda:{device}")
            return t.data_ptr(), t
    t0 = time.perf_counter()
    b = IvfBuilder(d, nlist, device)
    n_sample = int(min(n, nlist * points_per_centroid)) if sample_rows is None else int(sample_rows)
    stride = max(1, n // n_sample)
    sample_ptr, sample_keep = alloc(n_sample * d * 2)
    fill_rows(sample_ptr, 0, n_sample, stride)
    train_ivf_centroids_device(b, sample_ptr, n_sample, niter=niter, seed=seed)
    cent = np.ascontiguousarray(b.centroids())
    del sample_keep
    _release_cached_device_memory()  # the arena allocated below needs the bytes a caching allocator would sit on
    t1 = time.perf_counter()
    # pass 1: list of every row (4 bytes per row stay on the device), list sizes
    lists_ptr, lists_keep = alloc(n * 4)
    rows_ptr, rows_keep = alloc(min(chunk, n) * d * 2)
    b.list_sizes(reset=True)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        fill_rows(rows_ptr, o, m, 1)
        b.assign_device(rows_ptr, m, lists_ptr + 4 * o)
    sizes = b.list_sizes()
    b.close()
    _release_cached_device_memory()
    t2 = time.perf_counter()
    # pass 2: scatter into the list-sorted arena
    index = Mi355xIndex(d, device=device, id_base=id_base)
    check(lib, lib.knnx_ivf_begin(index._h, nlist, cent.ctypes.data, sizes.ctypes.data), "knnx")  # pylint: disable=protected-access
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        fill_rows(rows_ptr, o, m, 1)
        check(lib, lib.knnx_ivf_add_assigned_device(index._h, C.c_void_p(rows_ptr), m, id_base + o, C.c_void_p(lists_ptr + 4 * o)), "knnx")  # pylint: disable=protected-access
    check(lib, lib.knnx_ivf_end(index._h), "knnx")  # pylint: disable=protected-access
    if keep_lists:  # tests / recall measurements: the list of every row (4 bytes per row to the host)
        index.ivf_lists = _download_i32(lists_ptr, n, device)
    del rows_keep, lists_keep
    _release_cached_device_memory()
    t3 = time.perf_counter()
    index.nprobe = min(nprobe, nlist)
    stats = {"train_s": t1 - t0, "assign_s": t2 - t1, "scatter_s": t3 - t2, "n_sample": n_sample, "list_sizes": sizes}
    return index, stats


def train_ivf_centroids(x_f16, nlist, niter=8, seed=0, device=0, max_points_per_centroid=256):
    """k-means with inner-product assignment (faiss Clustering with an IndexFlatIP quantiser): returns fp16 [nlist, d].
    The sample (<= nlist * max_points_per_centroid rows, like faiss) stays resident in HBM across the iterations."""
    x_f16 = np.asarray(x_f16)
    rng = np.random.default_rng(seed)
    n, d = x_f16.shape
    if n < nlist:
        raise ValueError(f"need at least nlist={nlist} training rows, got {n}")
    take = min(n, nlist * max_points_per_centroid)
    sample = x_f16[np.sort(rng.choice(n, take, replace=False))] if take < n else x_f16
    b = IvfBuilder(d, nlist, device)
    b.set_sample(sample)
    b.set_centroids(sample[rng.choice(sample.shape[0], nlist, replace=False)])
    for it in range(niter):
        sizes = b.update(b.assign_sample())
        if it < niter - 2 and nlist >= 16:  # split-and-merge: the smallest lists' centroids move into the largest lists
            cent = b.centroids().astype(np.float32)
            if rebalance_centroids(cent, sizes, rng):
                b.set_centroids(cent.astype(np.float16))
                continue
        empty = np.flatnonzero(sizes == 0)
        if empty.size:  # re-seed empty clusters on random points (faiss splits big clusters; any re-seed is valid)
            cent = b.centroids()
            cent[empty] = np.asarray(sample[rng.choice(sample.shape[0], empty.size, replace=False)], dtype=np.float16)
            b.set_centroids(cent)
    cent = b.centroids()
    b.close()
    return cent


def _positions_in_lists(lists, cursor):
    """Stable rank of every row inside its list, continuing from `cursor` (rows of earlier chunks); updates cursor."""
    order = np.argsort(lists, kind="stable")
    sl = lists[order]
    start = np.flatnonzero(np.r_[True, sl[1:] != sl[:-1]])
    run_len = np.diff(np.r_[start, sl.size])
    rank_sorted = np.arange(sl.size) - np.repeat(start, run_len)
    pos = np.empty(lists.size, dtype=np.int64)
    pos[order] = rank_sorted + cursor[sl]
    np.add.at(cursor, sl[start], run_len)
    return pos.astype(np.int32)


def _list_sizes(lists, nlist):
    sizes = np.bincount(lists, minlength=nlist).astype(np.int64)
    if sizes.shape[0] != nlist:
        raise ValueError("a list id is outside [0, nlist)")
    return sizes


def _ivf_begin(index, nlist, centroids, sizes):
    """knnx_ivf_begin on an index whose quantiser, if it has one, is set -> the padded centroids it was given."""
    cpad = np.ascontiguousarray(index._pad(np.asarray(centroids, dtype=np.float16)))  # pylint: disable=protected-access
    check(index._lib, index._lib.knnx_ivf_begin(index._h, nlist, cpad.ctypes.data, np.ascontiguousarray(sizes, dtype=np.int64).ctypes.data), "knnx")  # pylint: disable=protected-access
    return index


def _add_assigned_chunks(index, chunks, lists, nlist, id_base):
    """Rows (an iterator of (offset, fp16 rows)) into an index between knnx_ivf_begin and knnx_ivf_end: row offset + j gets id
    id_base + offset + j and the next free slot of list lists[offset + j] (an IVF-PQ / IVF-SQ8 index encodes it there)."""
    lib = index._lib  # pylint: disable=protected-access
    cursor = np.zeros(nlist, dtype=np.int64)
    for o, x in chunks:
        rows = np.ascontiguousarray(index._pad(np.asarray(x, dtype=np.float16)))  # pylint: disable=protected-access
        ls = np.ascontiguousarray(lists[o:o + rows.shape[0]], dtype=np.int32)
        pos = _positions_in_lists(ls, cursor)
        ids = np.arange(o, o + rows.shape[0], dtype=np.int64) + id_base
        check(lib, lib.knnx_ivf_add_assigned(index._h, rows.ctypes.data, rows.shape[0], ids.ctypes.data, ls.ctypes.data, pos.ctypes.data), "knnx")  # pylint: disable=protected-access


def _add_code_chunks(index, add_codes, codes, lists, lo, nlist, chunk, prepare=lambda c: c):
    """Saved codes (u8 [n, width], ids lo + row number) into an index between knnx_ivf_begin and knnx_ivf_end through the library's
    add_codes (knnx_ivfpq_add_codes / knnx_ivfsq_add_codes), `chunk` rows at a time."""
    lib = index._lib  # pylint: disable=protected-access
    cursor = np.zeros(nlist, dtype=np.int64)
    for o in range(0, codes.shape[0], chunk):
        c = np.ascontiguousarray(prepare(np.asarray(codes[o:o + chunk], dtype=np.uint8)))
        ls = np.ascontiguousarray(lists[o:o + chunk], dtype=np.int32)
        pos = _positions_in_lists(ls, cursor)
        ids = np.arange(lo + o, lo + o + c.shape[0], dtype=np.int64)
        check(lib, add_codes(index._h, c.ctypes.data, c.shape[0], ids.ctypes.data, ls.ctypes.data, pos.ctypes.data), "knnx")  # pylint: disable=protected-access


def _ivf_end(index, nlist, nprobe, centroids, id_base, n, lists=None):
    """knnx_ivf_end, then what every built IVF index carries: nprobe, its centroids and row range, the lists where they are known."""
    check(index._lib, index._lib.knnx_ivf_end(index._h), "knnx")  # pylint: disable=protected-access
    index.nprobe = min(int(nprobe), nlist)
    index.ivf_centroids, index.ivf_row_range = np.asarray(centroids, dtype=np.float16), (int(id_base), int(id_base) + int(n))
    if lists is not None:
        index.ivf_lists = lists
    return index


def _encode_chunks(begin, chunks, n, nlist, centroids, lists, nprobe, id_base):
    """Rows (an iterator of (offset, fp16 rows)) -> a compressed IVF index: begin(list sizes) makes the index and opens the build."""
    index = begin(_list_sizes(lists, nlist))
    _add_assigned_chunks(index, chunks, lists, nlist, id_base)
    return _ivf_end(index, nlist, nprobe, centroids, id_base, n, lists)


def _split_saved_rows(make, codes, lists, saved_range, nprobe, device, row_range, devices):
    """What load_index does with the saved rows [slo, shi) of a compressed index: all of them or `row_range` on one device, or an
    even split over `devices`.  make(codes, lists, first id, device) builds one index."""
    slo, shi = saved_range
    if devices is not None:
        if row_range is not None:
            raise ValueError("row_range and devices are mutually exclusive")
        G = len(devices)
        cuts = [slo + (shi - slo) * g // G for g in range(G + 1)]
        shards = [make(codes[cuts[g] - slo:cuts[g + 1] - slo], np.asarray(lists[cuts[g] - slo:cuts[g + 1] - slo]), cuts[g], devices[g])
                  for g in range(G)]
        sharded = ShardedMi355xIndex.from_shards(shards, cuts[:-1])
        sharded.nprobe = nprobe
        return sharded
    lo, hi = (slo, shi) if row_range is None else (int(row_range[0]), int(row_range[1]))
    if not slo <= lo <= hi <= shi:
        raise ValueError(f"row_range {row_range} is outside the saved shard's rows [{slo}, {shi})")
    return make(codes[lo - slo:hi - slo], np.asarray(lists[lo - slo:hi - slo]), lo, device)


def threshold_scan_entry(on):
    """What a saved IVF-PQ or IVF-SQ8 manifest says about the threshold-scan switch: {"threshold_scan": true} when it is on, nothing
    otherwise."""
    return {"threshold_scan": True} if on else {}


def read_threshold_scan(folder, man):
    """The threshold-scan switch of a saved IVF-PQ or IVF-SQ8 manifest: False for a manifest without the key (every folder written
    before the switch existed, and every index saved with it off), else the boolean it carries; anything but a boolean is refused."""
    v = man.get("threshold_scan", False)
    if not isinstance(v, bool):
        raise ValueError(f"{folder}: \"threshold_scan\" must be true or false, got {v!r}")
    return v


ivfpq_threshold_scan_entry = ivfsq_threshold_scan_entry = threshold_scan_entry
read_ivfpq_threshold_scan = read_ivfsq_threshold_scan = read_threshold_scan


def build_ivf_index(x_f16, nlist, nprobe=16, niter=8, seed=0, device=0, id_base=0, centroids=None, chunk=1 << 20):
    """fp16 rows [N, d] -> HBM-resident IVF-Flat index (ids = id_base + row number, like the flat index).  `x_f16` may be a
    numpy memmap: rows are streamed twice in chunks (assignment, then scatter into the list-sorted arena)."""
    n, d = x_f16.shape
    if centroids is None:
        centroids = train_ivf_centroids(x_f16, nlist, niter=niter, seed=seed, device=device)
    centroids = np.asarray(centroids).astype(np.float16)
    b = IvfBuilder(d, nlist, device)
    b.set_centroids(centroids)
    lists = np.empty(n, dtype=np.int32)
    for o in range(0, n, chunk):
        lists[o:o + chunk] = b.assign(x_f16[o:o + chunk])
    b.close()
    index = _ivf_begin(Mi355xIndex(d, device=device, id_base=id_base), nlist, centroids, np.bincount(lists, minlength=nlist))
    _add_assigned_chunks(index, ((o, x_f16[o:o + chunk]) for o in range(0, n, chunk)), lists, nlist, id_base)
    # (the lists are kept for tests / recall measurement, and for save_index(index, folder, embeddings_folder=...))
    return _ivf_end(index, nlist, nprobe, centroids, id_base, n, lists)


# ------------------------------------------------------------------------------------------------------------
# IVF-Flat from disk and back ("img_emb_*.npy -> resident shards"; row a17: the reference builds once,
# offline -- clip_index.py:12-66 -- and boots by reading the index file -- clip_back.py:589-596, 883-896)
# ------------------------------------------------------------------------------------------------------------
IVF_MANIFEST = "ivf_manifest.json"
IVF_FORMAT = "clip-retrieval_amd ivf-flat v1"


class FolderRows:
    """The rows of one `clip inference` output folder (`img_emb_{zfill}.npy`, writer.py:67-75: NPY v1, C order, fp16 [n_i, d]) as
    ONE virtual [n, d] matrix in partition order -- global row number = id = metadata row (clip_back.py:401-417) -- read through
    np.load(mmap_mode="r"), never resident as a whole."""

    def __init__(self, folder):
        self.folder = folder
        self.files = embedding_files(folder)
        self.shapes = []
        for f in self.files:
            a = np.load(f, mmap_mode="r")
            if a.ndim != 2:
                raise ValueError(f"{f}: expected a 2-D embedding matrix")
            self.shapes.append(tuple(int(v) for v in a.shape))
        self.d = self.shapes[0][1]
        if any(sh[1] != self.d for sh in self.shapes):
            raise ValueError("embedding files disagree on the dimension")
        self.starts = np.concatenate([[0], np.cumsum([sh[0] for sh in self.shapes])]).astype(np.int64)
        self.n = int(self.starts[-1])

    def rows(self, lo, hi):
        """fp16 [hi - lo, d] (a copy), possibly spanning several files."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.n:
            raise IndexError(f"rows [{lo}, {hi}) outside [0, {self.n})")
        parts = []
        f0 = int(np.searchsorted(self.starts, lo, side="right")) - 1
        for fi in range(max(f0, 0), len(self.files)):
            a0, a1 = max(lo, int(self.starts[fi])), min(hi, int(self.starts[fi + 1]))
            if a1 > a0:
                a = np.load(self.files[fi], mmap_mode="r")[a0 - int(self.starts[fi]):a1 - int(self.starts[fi])]
                parts.append(np.asarray(a, dtype=np.float16))
            if int(self.starts[fi + 1]) >= hi:
                break
        if not parts:
            return np.zeros((0, self.d), dtype=np.float16)
        return np.ascontiguousarray(parts[0]) if len(parts) == 1 else np.concatenate(parts)

    def chunks(self, lo, hi, chunk):
        for o in range(int(lo), int(hi), int(chunk)):
            yield o, self.rows(o, min(o + chunk, hi))

    def take(self, idx):
        """fp16 rows at sorted global row numbers `idx` (the k-means training sample)."""
        idx = np.asarray(idx, dtype=np.int64)
        out = np.empty((idx.size, self.d), dtype=np.float16)
        fi = np.searchsorted(self.starts, idx, side="right") - 1
        for f in np.unique(fi):
            sel = np.flatnonzero(fi == f)
            out[sel] = np.load(self.files[int(f)], mmap_mode="r")[idx[sel] - int(self.starts[int(f)])]
        return out

    def manifest(self):
        return {"folder": os.path.abspath(self.folder), "files": [[os.path.basename(f), sh[0]] for f, sh in zip(self.files, self.shapes)],
                "rows": self.n, "d": self.d}


def _scatter_into_ivf(src, lo, hi, centroids, lists, nprobe, device, chunk):
    """The second pass of an IVF build: rows [lo, hi) of `src` into a list-sorted arena on `device` (ids = global row numbers),
    given every row's list id.  Streams the rows once; no training, no assignment."""
    nlist, d = centroids.shape
    index = _ivf_begin(Mi355xIndex(d, device=device, id_base=lo), nlist, centroids, _list_sizes(lists, nlist))
    _add_assigned_chunks(index, ((o - lo, x) for o, x in src.chunks(lo, hi, chunk)), lists, nlist, lo)
    index = _ivf_end(index, nlist, nprobe, centroids, lo, hi - lo, lists)
    index.ivf_source = src
    return _remember_folder(index, src)


def _remember_folder(index, src):
    """What append_new_folder_rows needs of the folder an index was built from: where it is, and the name and row count of every
    partition file it held then."""
    index.ivf_folder, index.ivf_folder_files = src.folder, src.manifest()["files"]
    return index


def append_new_folder_rows(index, folder=None, chunk=1 << 22):
    """The reference keeps writing img_emb_N.npy partitions into the embeddings folder (`clip inference`): append the rows the folder
    gained since `index` was built from it (build_*_from_folder, or load_index of a folder that names its embeddings) -> their ids, the
    global row numbers.  The files the index was built from must still be a PREFIX of the folder's files, with the same names and row
    counts, and the index must reach the end of them (a shard that stops earlier cannot grow without renumbering); otherwise
    ValueError, before anything is touched.  The library assigns the rows (Mi355xIndex.ivf_append), so a following save_index +
    load_index gives the index a fresh build over the enlarged folder with the same centroids and quantiser gives.  `folder`: where the
    embeddings are now, if they moved.  The new rows go in `chunk` rows per call, and every call moves the arena once."""
    files = getattr(index, "ivf_folder_files", None)
    folder = folder or getattr(index, "ivf_folder", None)
    if files is None or folder is None:
        raise ValueError("append_new_folder_rows takes an index built from an embeddings folder (build_*_from_folder / load_index)")
    src = folder if isinstance(folder, FolderRows) else FolderRows(folder)
    now = src.manifest()["files"]
    files = [list(f) for f in files]
    if now[:len(files)] != files or src.d != index.d:
        raise ValueError(f"{src.folder}: the embedding files the index was built from changed (names / row counts / dimension): they must "
                         "still be the first files of the folder")
    old_n = sum(int(rows) for _, rows in files)
    lo, hi = getattr(index, "ivf_row_range", (0, old_n))
    if hi != old_n:
        raise ValueError(f"the index holds rows [{lo}, {hi}) of a folder that had {old_n}: only an index that reaches the end of its folder can grow")
    ids = [index.ivf_append(x) for _, x in src.chunks(old_n, src.n, chunk)]
    _remember_folder(index, src)
    if hasattr(index, "ivf_source"):
        index.ivf_source = src
    return np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)


def build_ivf_index_from_folder(path, nlist, nprobe=16, niter=8, seed=0, device=0, row_range=None, centroids=None,
                                max_points_per_centroid=256, chunk=1 << 20):
    """`clip inference` output folder -> HBM-resident IVF-Flat index, streaming the `.npy` partitions (never the whole shard in
    host memory; what `clip_index` / autofaiss do for the reference's index types, clip_index.py:12-66).
      pass 0  a strided sample of <= nlist * max_points_per_centroid rows -> spherical k-means on the GPU (train_ivf_centroids);
              `centroids=` skips it (all shards of a row-sharded index MUST share one set: train once, pass it to the others)
      pass 1  every row through the MFMA assignment kernel (knnx_ivfb_assign): 4 bytes of list id per row stay on the host
      pass 2  knnx_ivf_begin / add_assigned / end: the rows into the list-sorted, tile-padded arena
    `row_range=(lo, hi)`: one shard of a row-sharded index (ids stay global row numbers).  The result can be `save_index()`ed."""
    src = path if isinstance(path, FolderRows) else FolderRows(path)
    lo, hi = (0, src.n) if row_range is None else (int(row_range[0]), int(row_range[1]))
    if centroids is None:
        take = min(src.n, int(nlist) * int(max_points_per_centroid))  # sample the WHOLE folder, so that every shard trains the same
        idx = np.unique(np.linspace(0, src.n - 1, take).astype(np.int64))
        centroids = train_ivf_centroids(src.take(idx), nlist, niter=niter, seed=seed, device=device, max_points_per_centroid=max_points_per_centroid)
    centroids = np.asarray(centroids).astype(np.float16)
    b = IvfBuilder(src.d, nlist, device)
    b.set_centroids(centroids)
    lists = np.empty(hi - lo, dtype=np.int32)
    for o, x in src.chunks(lo, hi, chunk):
        lists[o - lo:o - lo + x.shape[0]] = b.assign(x)
    b.close()
    return _scatter_into_ivf(src, lo, hi, centroids, lists, nprobe, device, chunk)


def save_index(index, folder, embeddings_folder=None):
    """Write a built IVF-Flat index (build_ivf_index_from_folder, or build_ivf_index given `embeddings_folder`) so that a service
    boots WITHOUT k-means or assignment: `ivf_centroids.npy` (fp16 [nlist, d]), `ivf_lists.npy` (int32 list id of every row of the
    shard: 4 bytes per row) and `ivf_manifest.json` (format, d, nlist, nprobe, row range, and the embeddings folder with the name
    and row count of each partition file -- the rows themselves are not copied: the arena is rebuilt from them by one scatter
    pass).  The counterpart of the reference's `<indices>/image.index` written by clip_index (clip_index.py:12-66), read back by
    `load_index(folder)` in the place of clip_back.py:589-596."""
    import json  # pylint: disable=import-outside-toplevel

    if getattr(index, "pq_m", 0):
        return _save_ivfpq_index(index, folder, embeddings_folder)
    if getattr(index, "is_sq", False):
        return _save_ivfsq_index(index, folder)
    lists, cent = getattr(index, "ivf_lists", None), getattr(index, "ivf_centroids", None)
    src = getattr(index, "ivf_source", None)
    if lists is None or cent is None:
        raise ValueError("save_index takes an IVF-Flat index built by build_ivf_index_from_folder / build_ivf_index")
    if src is None:
        if embeddings_folder is None:
            raise ValueError("this index was built from an in-memory array: name the embeddings folder its rows can be re-read from")
        src = FolderRows(embeddings_folder)
    lo, hi = getattr(index, "ivf_row_range", (0, src.n))
    if hi - lo != lists.shape[0]:
        raise ValueError("list ids and row range disagree")
    os.makedirs(folder, exist_ok=True)
    np.save(os.path.join(folder, "ivf_centroids.npy"), np.asarray(cent, dtype=np.float16))
    np.save(os.path.join(folder, "ivf_lists.npy"), np.asarray(lists, dtype=np.int32))
    man = {"format": IVF_FORMAT, "d": int(index.d), "nlist": int(cent.shape[0]), "nprobe": int(index.nprobe), "row_range": [int(lo), int(hi)],
           "embeddings": src.manifest(), "embeddings_relative": os.path.relpath(os.path.abspath(src.folder), os.path.abspath(folder))}
    tmp = os.path.join(folder, IVF_MANIFEST + ".part")
    with open(tmp, "w", encoding="utf-8") as f:
        json.dump(man, f, indent=1)
    os.replace(tmp, os.path.join(folder, IVF_MANIFEST))  # the manifest appears last: a folder without it is not an index
    return man


def read_ivf_manifest(folder, embeddings_folder=None):
    """(manifest dict, FolderRows of the embeddings it names) -- the embeddings are looked for at the recorded relative path
    first (the index folder and the embeddings usually move together), then at the absolute one; their file names and row
    counts must still be what they were when the index was built (ids are row numbers)."""
    import json  # pylint: disable=import-outside-toplevel

    with open(os.path.join(folder, IVF_MANIFEST), encoding="utf-8") as f:
        man = json.load(f)
    if man.get("format") != IVF_FORMAT:
        raise ValueError(f"{folder}: unknown index format {man.get('format')!r}")
    cands = [embeddings_folder] if embeddings_folder else [os.path.normpath(os.path.join(folder, man["embeddings_relative"])), man["embeddings"]["folder"]]
    src = None
    for c in cands:
        if c and os.path.isdir(c) and glob.glob(os.path.join(c, "*.npy")):
            src = FolderRows(c)
            break
    if src is None:
        raise FileNotFoundError(f"{folder}: the embeddings this index was built from are not at {cands}")
    if src.manifest()["files"] != man["embeddings"]["files"] or src.d != man["d"]:
        raise ValueError(f"{src.folder}: the embedding files changed since the index was built (names / row counts / dimension)")
    return man, src


def _load_ivf_index(folder, device=0, row_range=None, devices=None, embeddings_folder=None, chunk=1 << 20):
    man, src = read_ivf_manifest(folder, embeddings_folder)
    cent = np.load(os.path.join(folder, "ivf_centroids.npy"))
    lists = np.load(os.path.join(folder, "ivf_lists.npy"), mmap_mode="r")
    slo, shi = man["row_range"]
    if cent.shape != (man["nlist"], man["d"]) or lists.shape[0] != shi - slo:
        raise ValueError(f"{folder}: sidecar files disagree with the manifest")
    if devices is not None:
        if row_range is not None:
            raise ValueError("row_range and devices are mutually exclusive")
        G = len(devices)
        cuts = [slo + (shi - slo) * g // G for g in range(G + 1)]
        shards = [_scatter_into_ivf(src, cuts[g], cuts[g + 1], cent, np.asarray(lists[cuts[g] - slo:cuts[g + 1] - slo]), man["nprobe"], devices[g], chunk)
                  for g in range(G)]
        sharded = ShardedMi355xIndex.from_shards(shards, cuts[:-1])
        sharded.nprobe = man["nprobe"]
        return sharded
    lo, hi = (slo, shi) if row_range is None else (int(row_range[0]), int(row_range[1]))
    if not slo <= lo <= hi <= shi:
        raise ValueError(f"row_range {row_range} is outside the saved shard's rows [{slo}, {shi})")
    return _scatter_into_ivf(src, lo, hi, cent, np.asarray(lists[lo - slo:hi - slo]), man["nprobe"], device, chunk)


# ------------------------------------------------------------------------------------------------------------
# IVF-PQ (faiss IndexIVFPQ(IndexFlatIP(d), d, nlist, M, 8), METRIC_INNER_PRODUCT, by_residual): what autofaiss builds for large
# corpora (clip_index.py:12-66; the reference notebook's OPQ256_768,IVF16384_HNSW32,PQ256x8 without HNSW; OPQ: train_opq below).  The coarse
# quantiser is the IVF-Flat one; every row is kept as M code bytes (csrc/knn_pq_kernels.hip), so 1 B x 768 fits one GPU.
# ------------------------------------------------------------------------------------------------------------
PQ_SAMPLE_ROWS = 256 * 256  # rows of the codebook training sample (faiss: 256 x ksub)
IVFPQ_MANIFEST = "ivf_pq_manifest.json"
IVFPQ_ROTATION = "ivf_pq_rotation.npy"
IVFPQ_FORMAT = "clip-retrieval_amd ivf-pq v1"


def _f16_padded(x, dpad):
    x = np.asarray(x)
    if x.dtype != np.float16:
        x = x.astype(np.float16)
    if x.shape[1] != dpad:
        out = np.zeros((x.shape[0], dpad), dtype=np.float16)
        out[:, : x.shape[1]] = x
        x = out
    return np.ascontiguousarray(x)


class PqBuilder:
    """Codebook training on one GPU (knnx_pqb_* of include/knnx.h): the sample rows, their lists and the coarse centroids stay
    resident; lloyd() = one iteration of the M L2 k-means (device assignment, host counting sort, fixed-order device mean)."""

    def __init__(self, d, M, device=0):
        self._lib = load_library()
        self.d, self.M, self.device = int(d), int(M), int(device)
        self._dpad = (self.d + 255) // 256 * 256
        h = C.c_void_p()
        check(self._lib, self._lib.knnx_pqb_create(self.device, self._dpad, self.M, C.byref(h)), "knnx")
        self._h = h
        self.n_sample = 0

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.knnx_pqb_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass

    def set_sample(self, x_f16, lists, centroids):
        x = _f16_padded(x_f16, self._dpad)
        ls = np.ascontiguousarray(lists, dtype=np.int32)
        c = _f16_padded(centroids, self._dpad)
        assert ls.shape[0] == x.shape[0]
        self.n_sample = x.shape[0]
        check(self._lib, self._lib.knnx_pqb_set_sample(self._h, x.ctypes.data, ls.ctypes.data, x.shape[0], c.ctypes.data, c.shape[0]), "knnx")

    def set_sample_device(self, rows_ptr, lists_ptr, n, centroids):
        """Borrow n fp16 device rows [n, d_padded] with their int32 device list ids (the caller keeps the rows alive)."""
        c = _f16_padded(centroids, self._dpad)
        self.n_sample = int(n)
        check(self._lib, self._lib.knnx_pqb_set_sample_device(self._h, C.c_void_p(rows_ptr), C.c_void_p(lists_ptr), int(n), c.ctypes.data,
                                                              c.shape[0]), "knnx")

    def seed_from_sample(self, mj, sample_rows):
        """codebook entry mj[i] (= m * 256 + j) := residual sub-vector m of sample row sample_rows[i]."""
        a = np.ascontiguousarray(mj, dtype=np.int32)
        r = np.ascontiguousarray(sample_rows, dtype=np.int64)
        assert a.shape == r.shape
        check(self._lib, self._lib.knnx_pqb_seed_from_sample(self._h, a.ctypes.data, r.ctypes.data, a.size), "knnx")

    def set_codebooks(self, cb):
        cb = np.ascontiguousarray(cb, dtype=np.float32)
        assert cb.size == 256 * self._dpad
        check(self._lib, self._lib.knnx_pqb_set_codebooks(self._h, cb.ctypes.data), "knnx")

    def codebooks(self):
        out = np.empty((self.M, 256, self._dpad // self.M), dtype=np.float32)
        check(self._lib, self._lib.knnx_pqb_get_codebooks(self._h, out.ctypes.data), "knnx")
        return out

    def lloyd(self, want_codes=False):
        """One iteration; returns (cluster sizes int64 [M, 256], the iteration's codes u8 [n, M] or None)."""
        sizes = np.empty((self.M, 256), dtype=np.int64)
        codes = np.empty((self.n_sample, self.M), dtype=np.uint8) if want_codes else None
        check(self._lib, self._lib.knnx_pqb_lloyd(self._h, codes.ctypes.data if want_codes else None, sizes.ctypes.data), "knnx")
        return sizes, codes


def train_pq_codebooks(builder, niter=10, seed=0):
    """M independent L2 k-means of 256 over the builder's resident residual sample: initial codewords are residual sub-vectors of
    distinct random sample rows (per sub-quantiser), then `niter` Lloyd iterations; between iterations an empty cluster is re-seeded
    on a random sample row (a host step, as in the IVF-Flat trainer).  Returns the codebooks f32 [M, 256, d_padded / M]."""
    rng = np.random.default_rng(seed)
    n, M = builder.n_sample, builder.M
    if n < 256:
        raise ValueError(f"PQ training needs at least 256 sample rows, got {n}")
    rows = np.concatenate([np.sort(rng.choice(n, 256, replace=False)) for _ in range(M)])
    builder.seed_from_sample(np.arange(M * 256), rows)
    for it in range(niter):
        sizes, _ = builder.lloyd()
        empty = np.flatnonzero(sizes.reshape(-1) == 0)
        if empty.size and it < niter - 1:
            builder.seed_from_sample(empty, rng.choice(n, empty.size))
    return builder.codebooks()


# ------------------------------------------------------------------------------------------------------------
# OPQ: the learned rotation in front of IVF-PQ (faiss OPQMatrix, d_out = d_in; what autofaiss puts in front of every IVF-PQ index,
# clip_index.py:12-66).  The device does the arithmetic over rows (rotation: the MFMA kernel knn_rotate_kernel; PQ Lloyd: PqBuilder;
# X^T Y: xty_kernel); the host takes the SVD of one d x d matrix per iteration.
# ------------------------------------------------------------------------------------------------------------
OPQ_SAMPLE_ROWS = 65536


def _pad_rotation(A, dpad):
    """[d, d] -> [dpad, dpad]: the zero pad columns of the rows map onto themselves."""
    A = np.asarray(A, dtype=np.float32)
    d = A.shape[0]
    if d == dpad:
        return np.ascontiguousarray(A)
    out = np.eye(dpad, dtype=np.float32)
    out[:d, :d] = A
    return out


def rotate_rows_device(A, rows_ptr, n, out_ptr, device=0, stream=None):
    """out[i] = fp16(A rows[i]) for n fp16 device rows [n, d_padded] (include/knnx.h: knnx_rotate_f16_device); A f32 [d_padded,
    d_padded]; out must not overlap rows.  Synchronous.  A f32 [d_out, d_in] with d_out > d_in (knnx_rotate_rect_f16_device): rows
    [n, d_in] -> out [n, d_out]."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    lib = load_library()
    st = C.c_void_p(stream) if stream else None
    if A.shape[0] != A.shape[1]:
        check(lib, lib.knnx_rotate_rect_f16_device(int(device), A.ctypes.data, C.c_void_p(int(rows_ptr)), int(n), A.shape[1], A.shape[0],
                                                   C.c_void_p(int(out_ptr)), st), "knnx")
        return
    check(lib, lib.knnx_rotate_f16_device(int(device), A.ctypes.data, C.c_void_p(int(rows_ptr)), int(n), A.shape[0], C.c_void_p(int(out_ptr)),
                                          st), "knnx")


def rotate_rows(A, x_f16, device=0, chunk=1 << 20):
    """Host rows fp16 [n, d] -> fp16 [n, d] rotated on the device, chunk by chunk (the assignment pass of the host builds, tests).
    A f32 [d_out, d] with d_out > d (d % 256 == 0): -> fp16 [n, d_out]."""
    import torch  # pylint: disable=import-outside-toplevel

    x_f16 = np.asarray(x_f16)
    n, d = x_f16.shape
    A = np.asarray(A, dtype=np.float32)
    if A.shape[0] != A.shape[1]:
        if A.shape[1] != d or d % 256 != 0:
            raise ValueError(f"a rotation {A.shape} takes rows of width {A.shape[1]} with d % 256 == 0, got rows of width {d}")
        out = np.empty((n, A.shape[0]), dtype=np.float16)
        for o in range(0, n, chunk):
            xt = torch.from_numpy(np.array(x_f16[o:o + chunk], dtype=np.float16)).to(f"cuda:{device}")  # (a copy: the source may be read-only)
            yt = torch.empty((xt.shape[0], A.shape[0]), dtype=torch.float16, device=xt.device)
            torch.cuda.synchronize(device)
            rotate_rows_device(A, xt.data_ptr(), xt.shape[0], yt.data_ptr(), device)
            out[o:o + chunk] = yt.cpu().numpy()
        return out
    dpad = (d + 255) // 256 * 256
    Ap = _pad_rotation(A, dpad)
    out = np.empty((n, d), dtype=np.float16)
    for o in range(0, n, chunk):
        xt = torch.from_numpy(_f16_padded(x_f16[o:o + chunk], dpad)).to(f"cuda:{device}")
        yt = torch.empty_like(xt)
        torch.cuda.synchronize(device)
        rotate_rows_device(Ap, xt.data_ptr(), xt.shape[0], yt.data_ptr(), device)
        out[o:o + chunk] = yt.cpu().numpy()[:, :d]
    return out


def opq_procrustes(G):
    """The orthonormal A (y = A x) that minimises sum_i ||A x_i - y_i||^2, from G = X^T Y = sum_i x_i y_i^T: with G = U S V^T, A = V U^T
    (faiss OPQMatrix::train takes the same SVD).  float64 on the host; G is d x d, d <= 1024."""
    U, _, Vt = np.linalg.svd(np.asarray(G, dtype=np.float64))
    return np.ascontiguousarray((U @ Vt).T.astype(np.float32))


def opq_initial_rotation(d, seed):
    """The seeded random orthonormal start: Q of the QR of a Gaussian matrix, columns signed so that R's diagonal is positive."""
    g = np.random.default_rng(seed).standard_normal((d, d))
    Q, R = np.linalg.qr(g)
    return np.ascontiguousarray((Q * np.sign(np.diag(R))[None, :]).astype(np.float32))


def train_opq_device(x_ptr, n, d, M, niter=8, pq_niter=4, seed=0, device=0):
    """faiss' non-parametric OPQ over n fp16 rows [n, d] ALREADY IN HBM (d % 256 == 0): from a seeded random orthonormal matrix, per
    iteration rotate the sample, train the M codebooks on the rotated rows (PqBuilder: one list with a zero centroid, so the
    "residual" is the row), decode, G = X^T decoded on the device, A = the Procrustes solution of its SVD.  Every device step sums in
    a fixed order: one seed, one matrix.  Returns A f32 [d, d]."""
    import torch  # pylint: disable=import-outside-toplevel

    assert d % 256 == 0, "device rows are padded (d % 256 == 0)"
    lib = load_library()
    dev = f"cuda:{device}"
    A = opq_initial_rotation(d, seed)
    y = torch.empty((n, d), dtype=torch.float16, device=dev)
    zeros = torch.zeros(n, dtype=torch.int32, device=dev)
    G = torch.empty((d, d), dtype=torch.float32, device=dev)
    cent0 = np.zeros((1, d), dtype=np.float16)
    m_idx = torch.arange(M, device=dev)[None, :]
    for it in range(niter):
        torch.cuda.synchronize(device)
        rotate_rows_device(A, x_ptr, n, y.data_ptr(), device)
        pb = PqBuilder(d, M, device)
        pb.set_sample_device(y.data_ptr(), zeros.data_ptr(), n, cent0)
        cb = train_pq_codebooks(pb, niter=pq_niter, seed=seed + it)
        _, codes = pb.lloyd(want_codes=True)  # (the assignment of this call is against `cb`; the update behind it is not used)
        pb.close()
        dec = torch.from_numpy(cb).to(dev)[m_idx, torch.from_numpy(codes).to(dev).long()].reshape(n, d).contiguous()
        torch.cuda.synchronize(device)
        check(lib, lib.knnx_xty_device(int(device), C.c_void_p(int(x_ptr)), C.c_void_p(dec.data_ptr()), int(n), int(d), C.c_void_p(G.data_ptr()),
                                       None), "knnx")
        A = opq_procrustes(G.cpu().numpy())
        del dec
    return A


def opq_embedding(d, d_out):
    """The zero-embedding E f32 [d_out, d] (E x = x followed by d_out - d zeros): rotating rows by it pads them on the device, exactly."""
    E = np.zeros((d_out, d), dtype=np.float32)
    E[np.arange(d), np.arange(d)] = 1.0
    return E


def _check_opq_dim(d, d_out):
    if d % 256 != 0 or d_out % 256 != 0 or not 256 <= d < d_out <= 1024:
        raise ValueError(f"an OPQ rotation with d_out != d needs both widths multiples of 256 and 256 <= d < d_out <= 1024 "
                         f"(got d = {d}, d_out = {d_out})")


def train_opq(x_f16, M, niter=8, pq_niter=4, seed=0, device=0, sample_rows=OPQ_SAMPLE_ROWS, d_out=None):
    """OPQ rotation for host rows fp16 [n, d] (a seeded sample of <= sample_rows of them): A f32 [d, d], orthonormal, y = A x.  See
    train_opq_device.  d_out > d (faiss OPQMatrix(d, M, d_out)): A f32 [d_out, d] with orthonormal columns -- faiss' recipe: the sample
    zero-padded to d_out, the square trainer at d_out, the first d columns of its matrix."""
    import torch  # pylint: disable=import-outside-toplevel

    x_f16 = np.asarray(x_f16)
    n, d = x_f16.shape
    take = min(n, int(sample_rows))
    sample = x_f16[np.sort(np.random.default_rng(seed + 2).choice(n, take, replace=False))] if take < n else x_f16
    if d_out is not None and int(d_out) != d:
        d_out = int(d_out)
        _check_opq_dim(d, d_out)
        xt = torch.from_numpy(_f16_padded(sample, d_out)).to(f"cuda:{device}")
        A = train_opq_device(xt.data_ptr(), take, d_out, M, niter=niter, pq_niter=pq_niter, seed=seed, device=device)
        # The comment below about arbitrary SVD blocks does not reach the columns kept here.  The padded rows are zero in columns
        # d .., so G = X^T Y has zero ROWS d ..: G = [G1; 0] with G1 [d, d_out].  The Procrustes matrix A = (U V^T)^T then has
        # A[:, :d] = the transposed polar factor of G1, which is unique as soon as G1 has rank d (a sample that spans its d columns);
        # everything the SVD is free to choose -- the completion of that factor to a square matrix -- sits in columns d .. of A, which
        # only ever multiply the zero pad and are dropped.  Orthonormal columns of a square orthonormal matrix stay orthonormal.
        return np.ascontiguousarray(A[:, :d])
    dpad = (d + 255) // 256 * 256
    xt = torch.from_numpy(_f16_padded(sample, dpad)).to(f"cuda:{device}")
    if dpad == d:
        return train_opq_device(xt.data_ptr(), take, d, M, niter=niter, pq_niter=pq_niter, seed=seed, device=device)
    # padded rows: the zero columns carry no variance, G is singular there and the SVD's choice on that block is arbitrary -- the
    # rotation is learned for a d_padded-wide problem and must be square in d, so such widths are refused rather than guessed
    raise ValueError(f"train_opq needs d % 256 == 0 (got {d}): pass rotation= for other widths")


def _resolve_rotation(x_sample, M, opq, rotation, seed, device, opq_dim=None):
    """opq / rotation / opq_dim arguments of the builders -> (A f32 [d, d] -- [opq_dim, d] with an opq_dim != d -- or None, seconds
    spent training it).  A given rotation says its own d_out (its row count); an opq_dim next to it must agree."""
    import time  # pylint: disable=import-outside-toplevel

    if rotation is not None:
        A = np.ascontiguousarray(rotation, dtype=np.float32)
        if opq_dim is not None and A.shape[0] != int(opq_dim):
            raise ValueError(f"rotation {A.shape} does not have opq_dim = {opq_dim} rows")
        if A.ndim != 2 or (A.shape[0] != A.shape[1] and A.shape[1] % 256 != 0):
            raise ValueError(f"a rotation with d_out != d needs d % 256 == 0, got {A.shape}")
        return A, 0.0
    if not opq:
        if opq_dim is not None:
            raise ValueError("opq_dim needs opq=True or rotation=")
        return None, 0.0
    t = time.perf_counter()
    A = train_opq(x_sample, M, seed=seed, device=device, d_out=opq_dim)
    return A, time.perf_counter() - t


def _rotation_out_dim(A, d):
    """Width of the space behind the rotation: its row count when it is rectangular, else d."""
    return int(A.shape[0]) if A is not None and A.shape[0] != A.shape[1] else int(d)


def train_ivfpq(x_f16, nlist, M, niter=8, pq_niter=10, seed=0, device=0, sample_rows=PQ_SAMPLE_ROWS, centroids=None,
                max_points_per_centroid=256, opq=False, rotation=None, opq_dim=None):
    """faiss IndexIVFPQ.train order: the coarse centroids first (the spherical k-means of train_ivf_centroids; `centroids=` skips it),
    then the M sub-quantisers on the residuals of a sample of <= sample_rows rows against their lists.  Returns (centroids fp16
    [nlist, d], codebooks f32 [M, 256, d_padded / M]).
    opq=True / rotation=A (f32 [d, d]): the order of faiss' IndexPreTransform.train -- the OPQ rotation first, on the raw rows
    (train_opq), then everything above on the ROTATED rows; returns (centroids, codebooks, A), both in the rotated space (`centroids=`
    are then centroids of the rotated space).  opq_dim=d_out (or a rotation [d_out, d]): the rotated space is d_out wide -- centroids
    fp16 [nlist, d_out], codebooks f32 [M, 256, d_out / M]."""
    x_f16 = np.asarray(x_f16)
    n, d = x_f16.shape
    A, _ = _resolve_rotation(x_f16, M, opq, rotation, seed, device, opq_dim)
    if A is not None:
        c, cb = train_ivfpq(rotate_rows(A, x_f16, device), nlist, M, niter=niter, pq_niter=pq_niter, seed=seed, device=device,
                            sample_rows=sample_rows, centroids=centroids, max_points_per_centroid=max_points_per_centroid)
        return c, cb, A
    if centroids is None:
        centroids = train_ivf_centroids(x_f16, nlist, niter=niter, seed=seed, device=device, max_points_per_centroid=max_points_per_centroid)
    centroids = np.asarray(centroids).astype(np.float16)
    rng = np.random.default_rng(seed + 1)
    take = min(n, int(sample_rows))
    sample = np.asarray(x_f16[np.sort(rng.choice(n, take, replace=False))] if take < n else x_f16, dtype=np.float16)
    ib = IvfBuilder(d, centroids.shape[0], device)
    ib.set_centroids(centroids)
    lists = ib.assign(sample)
    ib.close()
    b = PqBuilder(d, M, device)
    b.set_sample(sample, lists, centroids)
    cb = train_pq_codebooks(b, niter=pq_niter, seed=seed)
    b.close()
    return centroids, cb


def ivfpq_params_from_index_key(key, d):
    """A faiss index-factory string of the family autofaiss builds -- `OPQ{M}_{d_out},IVF{nlist}[_HNSW32],PQ{M}x8[,RFlat]`, the OPQ
    part optional -- for rows of width d -> the keyword arguments of build_ivfpq_index*: {"nlist", "M", "opq", "opq_dim", "refine"}
    (opq_dim is None when d_out == d).  The _HNSW32 suffix is accepted and ignored: the coarse quantiser here is flat.  Whatever
    cannot be served raises ValueError naming the part.  It parses; it does not choose an index."""
    import re  # pylint: disable=import-outside-toplevel

    d = int(d)
    parts = [p.strip() for p in str(key).split(",")]
    out = {"nlist": None, "M": None, "opq": False, "opq_dim": None, "refine": False}
    opq_m = None
    i = 0
    m = re.fullmatch(r"OPQ(\d+)(?:_(\d+))?", parts[i]) if parts else None
    if m:
        opq_m, d_out = int(m.group(1)), int(m.group(2)) if m.group(2) else d
        if d_out != d:
            try:
                _check_opq_dim(d, d_out)
            except ValueError as e:
                raise ValueError(f"index key part {parts[i]!r}: {e}") from None
            out["opq_dim"] = d_out
        out["opq"] = True
        i += 1
    m = re.fullmatch(r"IVF(\d+)(_HNSW\d+)?", parts[i]) if i < len(parts) else None
    if not m or int(m.group(1)) < 1:
        raise ValueError(f"index key part {parts[i] if i < len(parts) else ''!r}: expected IVF{{nlist}} or IVF{{nlist}}_HNSW32")
    out["nlist"] = int(m.group(1))
    i += 1
    m = re.fullmatch(r"PQ(\d+)(?:x(\d+))?", parts[i]) if i < len(parts) else None
    if not m:
        raise ValueError(f"index key part {parts[i] if i < len(parts) else ''!r}: expected PQ{{M}}x8")
    M, bits = int(m.group(1)), int(m.group(2)) if m.group(2) else 8
    if bits != 8:
        raise ValueError(f"index key part {parts[i]!r}: only 8-bit codes are served")
    dq = out["opq_dim"] or (d + 255) // 256 * 256
    ok = dq in (512, 768, 1024) if M == 256 else (M in (16, 32, 64, 128) and dq <= 1024 and dq % M == 0 and dq // M <= 64)
    if not ok:
        raise ValueError(f"index key part {parts[i]!r}: M = {M} does not fit a quantiser width of {dq} (M in 16, 32, 64, 128 dividing it, "
                         f"or M = 256 at 512, 768, 1024)")
    if opq_m is not None and opq_m != M:
        raise ValueError(f"index key part {parts[0]!r}: the OPQ block count {opq_m} differs from the PQ's M = {M}")
    out["M"] = M
    i += 1
    if i < len(parts) and parts[i] == "RFlat":
        out["refine"] = True
        i += 1
    if i < len(parts):
        raise ValueError(f"index key part {parts[i]!r}: not served (OPQ, IVF, PQ and RFlat parts only)")
    return out


def _ivfpq_begin(d, nlist, M, centroids, codebooks, sizes, device, id_base, rotation=None, refine=False, k_factor=1, threshold_scan=False):
    index = Mi355xIndex(d, device=device, id_base=id_base)
    dq = _rotation_out_dim(rotation, d)
    if dq != d:  # (a rectangular rotation says the quantiser width; every other index makes exactly the calls it always made)
        index.set_pq_out_dim(dq)
    index.set_pq_quantizer(M, codebooks)
    if rotation is not None:
        index.set_pq_rotation(rotation)
    if refine:
        index.set_pq_refine()
    index.k_factor = k_factor
    if threshold_scan:  # (off is the state of a new index: nothing is called for it)
        index.pq_threshold_scan = True
    if dq != d:
        cshape = index._pad(np.asarray(centroids, dtype=np.float16)).shape  # pylint: disable=protected-access
        if cshape != (nlist, dq):
            raise ValueError(f"centroids must be [{nlist}, {dq}] behind a rotation {rotation.shape}, got {cshape}")
    return _ivf_begin(index, nlist, centroids, sizes)


def _ivfpq_encode_chunks(chunks, n, d, nlist, M, centroids, codebooks, lists, nprobe, device, id_base, rotation=None, refine=False,
                         k_factor=1, threshold_scan=False):
    """Rows (an iterator of (offset, fp16 rows)) -> IVF-PQ index: every row is encoded into the next free slot of its list.  With a
    rotation the rows are the UN-ROTATED ones (the index rotates each chunk) and `lists` are those of the rotated rows."""
    return _encode_chunks(lambda sizes: _ivfpq_begin(d, nlist, M, centroids, codebooks, sizes, device, id_base, rotation, refine, k_factor,
                                                     threshold_scan), chunks, n, nlist, centroids, lists, nprobe, id_base)


def _assign_chunks(chunks, n, d, nlist, centroids, device, A):
    """List of every row (rotated by A first when there is one) -> (lists int32 [n], seconds spent rotating)."""
    import time  # pylint: disable=import-outside-toplevel

    b = IvfBuilder(_rotation_out_dim(A, d), nlist, device)
    b.set_centroids(centroids)
    lists = np.empty(n, dtype=np.int32)
    rotate_s = 0.0
    for o, x in chunks:
        if A is not None:
            t = time.perf_counter()
            x = rotate_rows(A, x, device)
            rotate_s += time.perf_counter() - t
        lists[o:o + x.shape[0]] = b.assign(x)
    b.close()
    return lists, rotate_s


def build_ivfpq_index(x_f16, nlist, M, nprobe=16, niter=8, pq_niter=10, seed=0, device=0, id_base=0, centroids=None, codebooks=None,
                      chunk=1 << 20, opq=False, rotation=None, refine=False, k_factor=1, threshold_scan=False, opq_dim=None):
    """fp16 rows [N, d] -> HBM-resident IVF-PQ index (ids = id_base + row number).  Trains (train_ivfpq) unless both `centroids` and
    `codebooks` are given; lists by the MFMA assignment kernel; codes by the device encoder.
    opq=True trains an OPQ rotation first (train_opq), rotation=A uses that one; centroids / codebooks, given or trained, are those of
    the rotated space.  The index keeps the rotation: it is searched with, and reconstructs, un-rotated vectors.
    refine=True keeps the fp16 rows next to the codes (Mi355xIndex.set_pq_refine) and re-scores k x k_factor candidates exactly.
    threshold_scan=True switches on k > 64 and range_search (Mi355xIndex.pq_threshold_scan; off by default).
    opq_dim=d_out with opq=True, or a rotation [d_out, d]: the rotation leads into a WIDER space (faiss OPQ{M}_{d_out}; d and d_out
    multiples of 256, d < d_out <= 1024) where centroids, codebooks and codes live; queries, reconstruct and the refine store stay d wide."""
    n, d = x_f16.shape
    A, _ = _resolve_rotation(x_f16, M, opq, rotation, seed, device, opq_dim)
    if centroids is None or codebooks is None:
        centroids, codebooks = train_ivfpq(x_f16, nlist, M, niter=niter, pq_niter=pq_niter, seed=seed, device=device, centroids=centroids,
                                           rotation=A)[:2]
    centroids = np.asarray(centroids).astype(np.float16)
    lists, rotate_s = _assign_chunks(((o, x_f16[o:o + chunk]) for o in range(0, n, chunk)), n, d, nlist, centroids, device, A)
    index = _ivfpq_encode_chunks(((o, x_f16[o:o + chunk]) for o in range(0, n, chunk)), n, d, nlist, M, centroids, codebooks, lists, nprobe,
                                 device, id_base, A, refine, k_factor, threshold_scan)
    index.rotate_s = rotate_s
    return index


def build_ivfpq_index_from_folder(path, nlist, M, nprobe=16, niter=8, pq_niter=10, seed=0, device=0, centroids=None, codebooks=None,
                                  max_points_per_centroid=256, chunk=1 << 20, opq=False, rotation=None, refine=False, k_factor=1,
                                  threshold_scan=False, opq_dim=None):
    """`clip inference` output folder (img_emb_*.npy) -> IVF-PQ index, streaming the partitions: training on a strided sample of the
    whole folder, then one assignment pass and one encoding pass.  The result can be save_index()ed (self-contained).  opq / rotation
    as in build_ivfpq_index (the rotation is trained on the same strided sample).  refine / k_factor as in build_ivfpq_index; a saved
    refine index is loaded from its folder PLUS these embeddings (save_index(index, folder, embeddings_folder=...)).  threshold_scan as
    in build_ivfpq_index; save_index records it.  opq_dim as in build_ivfpq_index."""
    src = path if isinstance(path, FolderRows) else FolderRows(path)
    A = None if rotation is None else _resolve_rotation(None, M, opq, rotation, seed, device, opq_dim)[0]
    if opq_dim is not None and A is None and not opq:
        raise ValueError("opq_dim needs opq=True or rotation=")
    if centroids is None or codebooks is None or (opq and A is None):
        take = min(src.n, max(int(nlist) * int(max_points_per_centroid), PQ_SAMPLE_ROWS))
        idx = np.unique(np.linspace(0, src.n - 1, take).astype(np.int64))
        sample = src.take(idx)
        A, _ = _resolve_rotation(sample, M, opq, A, seed, device, opq_dim)
        if centroids is None or codebooks is None:
            centroids, codebooks = train_ivfpq(sample, nlist, M, niter=niter, pq_niter=pq_niter, seed=seed, device=device,
                                               centroids=centroids, max_points_per_centroid=max_points_per_centroid, rotation=A)[:2]
    centroids = np.asarray(centroids).astype(np.float16)
    lists, rotate_s = _assign_chunks(src.chunks(0, src.n, chunk), src.n, src.d, nlist, centroids, device, A)
    index = _ivfpq_encode_chunks(src.chunks(0, src.n, chunk), src.n, src.d, nlist, M, centroids, codebooks, lists, nprobe, device, 0, A,
                                 refine, k_factor, threshold_scan)
    index.rotate_s = rotate_s
    index.embeddings_folder = src.folder if hasattr(src, "folder") else None
    return _remember_folder(index, src)


def build_ivfpq_index_device(fill_rows, n, d, nlist, M, nprobe=16, niter=8, pq_niter=10, seed=0, device=0, id_base=0, centroids=None,
                             codebooks=None, chunk=1 << 20, alloc=None, points_per_centroid=64, pq_sample_rows=PQ_SAMPLE_ROWS, opq=False,
                             rotation=None, opq_sample_rows=OPQ_SAMPLE_ROWS, refine=False, k_factor=1, threshold_scan=False, opq_dim=None):
    """IVF-PQ index over n rows PRODUCED ON THE GPU (`fill_rows(dst_ptr, row0, count, stride)` as in build_ivf_index_device): the
    fp16 corpus never exists whole -- training samples, then per chunk one assignment pass and one encoding pass; the index keeps
    M bytes per row.  Returns (index, stats dict).
    opq=True / rotation=A: the rotation is trained on a strided sample of raw rows (train_opq_device), every training sample and every
    chunk of the assignment pass is rotated into a second buffer of its size before it is used, and the encoding pass hands the index
    un-rotated chunks (it rotates them itself).  stats["rotate_s"]: the rotations of the assignment pass (those of the encoding pass
    are part of encode_s), stats["opq_s"]: training the rotation (part of train_s).
    refine / k_factor as in build_ivfpq_index: the index stores each generated chunk as it encodes it (the chunk is handed over once
    and never held a second time); stats["code_arena_bytes"] / stats["row_arena_bytes"]: what the index keeps in HBM.
    opq_dim=d_out / a rotation [d_out, d]: as in build_ivfpq_index; a chunk is still held once per width -- the generated rows d wide,
    their rotation d_out wide."""
    import time

    assert d % 256 == 0, "device builds take padded rows (d % 256 == 0)"
    lib = load_library()
    if alloc is None:
        def alloc(nbytes):
            import torch

            t = torch.empty(int(nbytes), dtype=torch.uint8, device=f"cuda:{device}")
            return t.data_ptr(), t
    t0 = time.perf_counter()
    A = None if rotation is None else _resolve_rotation(None, M, opq, rotation, seed, device, opq_dim)[0]
    if A is not None and A.shape[0] == A.shape[1]:
        A = _pad_rotation(A, d)
    if opq_dim is not None and A is None and not opq:
        raise ValueError("opq_dim needs opq=True or rotation=")
    opq_s = rotate_s = 0.0
    if A is None and opq:
        n_os = int(min(n, opq_sample_rows))
        os_ptr, os_keep = alloc(n_os * d * 2)
        fill_rows(os_ptr, 0, n_os, max(1, n // n_os))
        if opq_dim is not None and int(opq_dim) != d:  # faiss' recipe (train_opq): the sample zero-padded to d_out, the first d columns kept
            _check_opq_dim(d, int(opq_dim))
            pad_ptr, pad_keep = alloc(n_os * int(opq_dim) * 2)
            rotate_rows_device(opq_embedding(d, int(opq_dim)), os_ptr, n_os, pad_ptr, device)
            A = np.ascontiguousarray(train_opq_device(pad_ptr, n_os, int(opq_dim), M, seed=seed, device=device)[:, :d])
            del pad_keep
        else:
            A = train_opq_device(os_ptr, n_os, d, M, seed=seed, device=device)
        del os_keep
        _release_cached_device_memory()
        opq_s = time.perf_counter() - t0
    dq = _rotation_out_dim(A, d)  # the width behind the rotation: training samples, centroids, codebooks, the rotated chunk

    def rotated(ptr, count):  # -> (pointer to the rotated rows, their owner): a second buffer, or the rows themselves without a rotation
        if A is None:
            return ptr, None
        rp, rk = alloc(count * dq * 2)
        rotate_rows_device(A, ptr, count, rp, device)
        return rp, rk

    b = IvfBuilder(dq, nlist, device)
    if centroids is None:
        n_sample = int(min(n, nlist * points_per_centroid))
        sample_ptr, sample_keep = alloc(n_sample * d * 2)
        fill_rows(sample_ptr, 0, n_sample, max(1, n // n_sample))
        sample_ptr, sample_rot_keep = rotated(sample_ptr, n_sample)
        train_ivf_centroids_device(b, sample_ptr, n_sample, niter=niter, seed=seed)
        centroids = np.ascontiguousarray(b.centroids())
        del sample_keep, sample_rot_keep
    centroids = np.asarray(centroids).astype(np.float16)
    b.set_centroids(centroids)
    if codebooks is None:
        n_ps = int(min(n, pq_sample_rows))
        ps_ptr, ps_keep = alloc(n_ps * d * 2)
        pl_ptr, pl_keep = alloc(n_ps * 4)
        fill_rows(ps_ptr, 0, n_ps, max(1, n // n_ps))
        ps_ptr, ps_rot_keep = rotated(ps_ptr, n_ps)
        b.assign_device(ps_ptr, n_ps, pl_ptr)
        pb = PqBuilder(dq, M, device)
        pb.set_sample_device(ps_ptr, pl_ptr, n_ps, centroids)
        codebooks = train_pq_codebooks(pb, niter=pq_niter, seed=seed)
        pb.close()
        del ps_keep, ps_rot_keep, pl_keep
    _release_cached_device_memory()
    t1 = time.perf_counter()
    lists_ptr, lists_keep = alloc(n * 4)
    rows_ptr, rows_keep = alloc(min(chunk, n) * d * 2)
    rot_ptr, rot_keep = alloc(min(chunk, n) * dq * 2) if A is not None else (rows_ptr, None)
    b.list_sizes(reset=True)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        fill_rows(rows_ptr, o, m, 1)
        if A is not None:
            tr = time.perf_counter()
            rotate_rows_device(A, rows_ptr, m, rot_ptr, device)
            rotate_s += time.perf_counter() - tr
        b.assign_device(rot_ptr, m, lists_ptr + 4 * o)
    sizes = b.list_sizes()
    b.close()
    del rot_keep
    t2 = time.perf_counter()
    index = _ivfpq_begin(d, nlist, M, centroids, codebooks, sizes, device, id_base, A, refine, k_factor, threshold_scan)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        fill_rows(rows_ptr, o, m, 1)
        check(lib, lib.knnx_ivf_add_assigned_device(index._h, C.c_void_p(rows_ptr), m, id_base + o, C.c_void_p(lists_ptr + 4 * o)), "knnx")  # pylint: disable=protected-access
    index = _ivf_end(index, nlist, nprobe, centroids, id_base, n)
    del rows_keep, lists_keep
    _release_cached_device_memory()
    t3 = time.perf_counter()
    code_bytes, row_bytes = index.pq_arena_bytes()
    stats = {"train_s": t1 - t0, "assign_s": t2 - t1, "encode_s": t3 - t2, "list_sizes": sizes, "bytes_per_row": M + 12 + (2 * d if refine else 0),
             "rotate_s": rotate_s, "opq_s": opq_s, "code_arena_bytes": code_bytes, "row_arena_bytes": row_bytes}
    return index, stats


def _save_ivfpq_index(index, folder, embeddings_folder=None):
    """The self-contained IVF-PQ folder: ivf_pq_centroids.npy (fp16 [nlist, d]), ivf_pq_codebooks.npy (f32 [M, 256, d_padded / M]),
    ivf_pq_codes.npy (u8 [n, M] in id order), ivf_pq_lists.npy (int32 [n]) and ivf_pq_manifest.json (written last); an index with an
    OPQ rotation adds ivf_pq_rotation.npy (f32 [d, d]) and "opq": true in the manifest; one whose quantiser space is wider than its
    rows also "d_out" (only then), and its rotation file is f32 [d_out, d], its centroids [nlist, d_out].  An index with a refine store adds "refine": true,
    "k_factor" and the embeddings folder (as save_index does for IVF-Flat) to the manifest: the rows are not written a second time, the
    folder is loaded together with the embeddings.  An index with the threshold scan switched on adds "threshold_scan": true (only
    then: every other folder is what it always was)."""
    import json  # pylint: disable=import-outside-toplevel

    cent = getattr(index, "ivf_centroids", None)
    if cent is None:
        raise ValueError("save_index takes an IVF-PQ index built by build_ivfpq_index* / load_index")
    src = None
    if index.pq_refine:
        src = embeddings_folder or getattr(index, "embeddings_folder", None)
        if src is None:
            raise ValueError("this IVF-PQ index has a refine store: name the embeddings folder its rows can be re-read from")
        src = src if isinstance(src, FolderRows) else FolderRows(src)
    codes, lists = index.pq_codes()
    lo, hi = getattr(index, "ivf_row_range", (0, codes.shape[0]))
    os.makedirs(folder, exist_ok=True)
    np.save(os.path.join(folder, "ivf_pq_centroids.npy"), np.asarray(cent, dtype=np.float16))
    np.save(os.path.join(folder, "ivf_pq_codebooks.npy"), index.pq_codebooks())
    np.save(os.path.join(folder, "ivf_pq_codes.npy"), codes)
    np.save(os.path.join(folder, "ivf_pq_lists.npy"), lists)
    man = {"format": IVFPQ_FORMAT, "d": int(index.d), "nlist": int(cent.shape[0]), "M": int(index.pq_m), "nprobe": int(index.nprobe),
           "row_range": [int(lo), int(hi)]}
    rot = index.pq_rotation()
    if rot is not None:  # (only then: a folder of an index without a rotation is what it always was)
        np.save(os.path.join(folder, IVFPQ_ROTATION), rot)
        man["opq"] = True
    man.update(ivfpq_out_dim_entry(index.d, index.pq_out_dim))
    if src is not None:
        if src.n < hi or src.d != index.d:
            raise ValueError(f"{src.folder}: {src.n} rows of width {src.d} cannot hold rows [{lo}, {hi}) of width {index.d}")
        man.update({"refine": True, "k_factor": int(index.k_factor), "embeddings": src.manifest(),
                    "embeddings_relative": os.path.relpath(os.path.abspath(src.folder), os.path.abspath(folder))})
    man.update(ivfpq_threshold_scan_entry(index.pq_threshold_scan))
    tmp = os.path.join(folder, IVFPQ_MANIFEST + ".part")
    with open(tmp, "w", encoding="utf-8") as f:
        json.dump(man, f, indent=1)
    os.replace(tmp, os.path.join(folder, IVFPQ_MANIFEST))
    return man


def ivfpq_out_dim_entry(d, d_out):
    """What a saved IVF-PQ manifest says about the quantiser width: {"d_out": d_out} when it differs from d, nothing otherwise."""
    return {"d_out": int(d_out)} if int(d_out) != int(d) else {}


def read_ivfpq_out_dim(folder, man):
    """The quantiser width of a saved IVF-PQ manifest: d for a manifest without "d_out" (every folder written before the key
    existed, and every index whose two widths agree), else the integer it carries -- which must obey the width rule and come with
    "opq": true, since only a rotation leads from d to d_out."""
    d = int(man["d"])
    if "d_out" not in man:
        return d
    v = man["d_out"]
    if not isinstance(v, int) or isinstance(v, bool) or v % 256 != 0 or d % 256 != 0 or not 256 <= d < v <= 1024:
        raise ValueError(f"{folder}: \"d_out\" must be a multiple of 256 with 256 <= d < d_out <= 1024 and d % 256 == 0, got d = {d}, "
                         f"d_out = {v!r}")
    if not man.get("opq", False):
        raise ValueError(f"{folder}: the manifest carries \"d_out\": {v} but does not say \"opq\": true (the rotation is what leads there)")
    return v


def read_ivfpq_rotation(folder, man):
    """The rotation a saved IVF-PQ folder carries: None for a manifest without "opq" (every folder written before the rotation
    existed), f32 [d, d] otherwise.  The flag and the file go together: either one without the other is refused.  A manifest with
    "d_out" carries f32 [d_out, d]; that shape is accepted only with the key, and the key only with that shape."""
    path = os.path.join(folder, IVFPQ_ROTATION)
    if not man.get("opq", False):
        if os.path.exists(path):
            raise ValueError(f"{folder}: {IVFPQ_ROTATION} is present but the manifest does not say \"opq\": true")
        if "d_out" in man:
            read_ivfpq_out_dim(folder, man)  # (raises: the key without the flag)
        return None
    if not os.path.isfile(path):
        raise ValueError(f"{folder}: the manifest says \"opq\": true but {IVFPQ_ROTATION} is missing")
    rot = np.load(path)
    d = int(man["d"])
    dq = read_ivfpq_out_dim(folder, man)
    if rot.shape != (dq, d) or rot.dtype != np.float32:
        raise ValueError(f"{folder}: {IVFPQ_ROTATION} must be float32 [{dq}, {d}], got {rot.dtype} {rot.shape}")
    return rot


def read_ivfpq_refine(folder, man, embeddings_folder=None):
    """The refine rules of a saved IVF-PQ manifest: (False, 1, None) for a manifest without "refine" (every folder written before the
    refine store existed, and every plain index since: self-contained), else (True, k_factor, FolderRows of the embeddings).  The
    embeddings are looked for at `embeddings_folder`, or at the recorded relative path, then at the absolute one; the flag without
    reachable embeddings, or embeddings whose files changed, are refused.  Touches no device."""
    if not man.get("refine", False):
        if "k_factor" in man:
            raise ValueError(f"{folder}: the manifest carries \"k_factor\" but does not say \"refine\": true")
        return False, 1, None
    kf = man.get("k_factor", 1)
    if not isinstance(kf, int) or isinstance(kf, bool) or not 1 <= kf <= 512:
        raise ValueError(f"{folder}: \"k_factor\" must be an integer in 1 .. 512, got {kf!r}")
    emb = man.get("embeddings")
    if not isinstance(emb, dict) or "files" not in emb:
        raise ValueError(f"{folder}: the manifest says \"refine\": true but names no embeddings")
    cands = [embeddings_folder] if embeddings_folder else [os.path.normpath(os.path.join(folder, man.get("embeddings_relative", "."))),
                                                            emb.get("folder")]
    src = None
    for c in cands:
        if c and os.path.isdir(c) and glob.glob(os.path.join(c, "*.npy")) and not os.path.isfile(os.path.join(c, IVFPQ_MANIFEST)):
            src = FolderRows(c)
            break
    if src is None:
        raise FileNotFoundError(f"{folder}: this IVF-PQ index has a refine store (\"refine\": true) and needs the embeddings it was built "
                                f"from; they are not at {cands} (pass embeddings_folder=)")
    if src.manifest()["files"] != emb["files"] or src.d != man["d"]:
        raise ValueError(f"{src.folder}: the embedding files changed since the index was built (names / row counts / dimension)")
    return True, kf, src


def _ivfpq_refine_from_rows(src, codes, lists, lo, cent, cb, M, nprobe, device, k_factor, chunk=1 << 20, rotation=None):
    """A saved refine index: rows [lo, lo + n) of the embeddings are stored AND re-encoded with the saved centroids, codebooks,
    rotation and lists; the codes that come out must be the saved ones."""
    n = codes.shape[0]
    index = _ivfpq_encode_chunks(((o - lo, x) for o, x in src.chunks(lo, lo + n, chunk)), n, src.d, cent.shape[0], M, cent, cb,
                                 np.asarray(lists, dtype=np.int32), nprobe, device, lo, rotation, True, k_factor)
    got = index.pq_codes()[0]
    if not np.array_equal(got, np.asarray(codes)):
        bad = int((got != np.asarray(codes)).any(axis=1).sum())
        index.close()
        raise ValueError(f"{bad} of {n} rows of {src.folder} do not encode to the saved ivf_pq_codes.npy: the embeddings or the codes changed")
    index.embeddings_folder = src.folder
    return _remember_folder(index, src)


def _ivfpq_from_codes(codes, lists, lo, cent, cb, M, nprobe, device, chunk=1 << 20, rotation=None):
    nlist, d = cent.shape
    if rotation is not None:  # (behind a rectangular rotation the centroids are d_out wide; the index is as wide as the rotation's input)
        d = rotation.shape[1]
    index = _ivfpq_begin(d, nlist, M, cent, cb, np.bincount(lists, minlength=nlist).astype(np.int64), device, lo, rotation)
    _add_code_chunks(index, index._lib.knnx_ivfpq_add_codes, codes, lists, lo, nlist, chunk)  # pylint: disable=protected-access
    return _ivf_end(index, nlist, nprobe, cent, lo, codes.shape[0], np.asarray(lists, dtype=np.int32))


def _load_ivfpq_index(folder, device=0, row_range=None, devices=None, embeddings_folder=None):
    import json  # pylint: disable=import-outside-toplevel

    with open(os.path.join(folder, IVFPQ_MANIFEST), encoding="utf-8") as f:
        man = json.load(f)
    if man.get("format") != IVFPQ_FORMAT:
        raise ValueError(f"{folder}: unknown index format {man.get('format')!r}")
    cent = np.load(os.path.join(folder, "ivf_pq_centroids.npy"))
    cb = np.load(os.path.join(folder, "ivf_pq_codebooks.npy"))
    codes = np.load(os.path.join(folder, "ivf_pq_codes.npy"), mmap_mode="r")
    lists = np.load(os.path.join(folder, "ivf_pq_lists.npy"), mmap_mode="r")
    rot = read_ivfpq_rotation(folder, man)
    refine, kf, src = read_ivfpq_refine(folder, man, embeddings_folder)
    thr_scan = read_ivfpq_threshold_scan(folder, man)
    slo, shi = man["row_range"]
    M = int(man["M"])

    def make(c, ls, lo_, dev):
        if refine:
            ix = _ivfpq_refine_from_rows(src, c, ls, lo_, cent, cb, M, man["nprobe"], dev, kf, rotation=rot)
        else:
            ix = _ivfpq_from_codes(c, ls, lo_, cent, cb, M, man["nprobe"], dev, rotation=rot)
        if thr_scan:
            ix.pq_threshold_scan = True
        return ix

    if cent.shape != (man["nlist"], read_ivfpq_out_dim(folder, man)) or codes.shape != (shi - slo, M) or lists.shape[0] != shi - slo:
        raise ValueError(f"{folder}: the IVF-PQ files disagree with the manifest")
    return _split_saved_rows(make, codes, lists, (slo, shi), man["nprobe"], device, row_range, devices)


# ------------------------------------------------------------------------------------------------------------
# IVF-SQ8 (faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_8bit, METRIC_INNER_PRODUCT), not residual; the factory string
# "IVF{nlist},SQ8"): one code byte per dimension (csrc/knn_sq_kernels.hip) -- d + 12 bytes per padded row against IVF-Flat's 2 d + 12,
# with a ranking that is practically IVF-Flat's.  The coarse quantiser and the list layout are the IVF-Flat ones; the builders mirror
# the IVF-PQ ones.
# ------------------------------------------------------------------------------------------------------------
IVFSQ_MANIFEST = "ivf_sq_manifest.json"
IVFSQ_FORMAT = "clip-retrieval_amd ivf-sq8 v1"


def train_sq_ranges(x, n=None, d=None, device=0, chunk=1 << 20):
    """The SQ8 quantiser of a training set (faiss ScalarQuantizer RS_minmax with argument 0): per-column (vmin, vdiff = vmax - vmin),
    f32 [d], by the column min / max kernel (knnx_colminmax_device).  `x`: fp16 rows [n, d] on the host (uploaded chunk by chunk), or
    the device address of n fp16 rows of width d (then name n and d).  Min and max do not depend on the order of the rows, so the
    result is that of x.astype(float32).min(0) / .max(0), bit for bit."""
    lib = load_library()
    if isinstance(x, (int, np.integer)):
        n, d = int(n), int(d)
        vmin, vmax = np.empty(d, dtype=np.float32), np.empty(d, dtype=np.float32)
        check(lib, lib.knnx_colminmax_device(int(device), C.c_void_p(int(x)), n, d, vmin.ctypes.data, vmax.ctypes.data, None), "knnx")
        return vmin, vmax - vmin
    import torch  # pylint: disable=import-outside-toplevel

    x = np.asarray(x)
    if x.ndim != 2 or x.shape[0] == 0:
        raise ValueError(f"train_sq_ranges takes rows [n, d] with n > 0, got {x.shape}")
    d = x.shape[1]
    vmin, vmax = np.full(d, np.inf, dtype=np.float32), np.full(d, -np.inf, dtype=np.float32)
    a, b = np.empty(d, dtype=np.float32), np.empty(d, dtype=np.float32)
    for o in range(0, x.shape[0], chunk):
        t = torch.from_numpy(np.ascontiguousarray(x[o:o + chunk], dtype=np.float16)).to(f"cuda:{device}")
        torch.cuda.synchronize(device)
        check(lib, lib.knnx_colminmax_device(int(device), C.c_void_p(t.data_ptr()), t.shape[0], d, a.ctypes.data, b.ctypes.data, None), "knnx")
        vmin, vmax = np.minimum(vmin, a), np.maximum(vmax, b)
        del t
    return vmin, vmax - vmin


def ivfsq_params_from_index_key(key):
    """The faiss index-factory string "IVF{nlist}[_HNSW32],SQ8" -> {"nlist": nlist}, the keyword argument of build_ivfsq_index*.  The
    _HNSW32 suffix is accepted and ignored (the coarse quantiser here is flat).  Whatever cannot be served -- another bit width (SQ4,
    SQ6, SQfp16), a pre-transform, a refine stage -- raises ValueError naming the part.  It parses; it does not choose an index."""
    import re  # pylint: disable=import-outside-toplevel

    parts = [p.strip() for p in str(key).split(",")]
    m = re.fullmatch(r"IVF(\d+)(_HNSW\d+)?", parts[0]) if parts else None
    if not m or int(m.group(1)) < 1:
        raise ValueError(f"index key part {parts[0] if parts else ''!r}: expected IVF{{nlist}} or IVF{{nlist}}_HNSW32")
    if len(parts) < 2 or parts[1] != "SQ8":
        raise ValueError(f"index key part {parts[1] if len(parts) > 1 else ''!r}: expected SQ8 (the 8-bit scalar quantiser is the only one served)")
    if len(parts) > 2:
        raise ValueError(f"index key part {parts[2]!r}: not served (IVF and SQ8 parts only)")
    return {"nlist": int(m.group(1))}


def ivfsq_manifest(d, nlist, nprobe, row_range):
    """The manifest of a saved IVF-SQ8 folder (kind "ivfsq")."""
    return {"format": IVFSQ_FORMAT, "kind": "ivfsq", "d": int(d), "nlist": int(nlist), "nprobe": int(nprobe),
            "row_range": [int(row_range[0]), int(row_range[1])]}


def check_ivfsq_manifest(man, where=""):
    """A manifest read back: the format and the kind must be this one's, the numbers consistent.  Returns it."""
    if man.get("format") != IVFSQ_FORMAT or man.get("kind") != "ivfsq":
        raise ValueError(f"{where}: unknown index format {man.get('format')!r} / kind {man.get('kind')!r}")
    lo, hi = man["row_range"]
    if not (int(man["d"]) > 0 and int(man["nlist"]) > 0 and 0 <= int(lo) <= int(hi) and int(man["nprobe"]) >= 1):
        raise ValueError(f"{where}: inconsistent IVF-SQ8 manifest {man}")
    return man


def _ivfsq_begin(d, nlist, centroids, ranges, sizes, device, id_base, threshold_scan=False):
    index = Mi355xIndex(d, device=device, id_base=id_base)
    index.set_sq_quantizer(*ranges)
    if threshold_scan:  # (off is the state of a new index: nothing is called for it)
        index.sq_threshold_scan = True
    return _ivf_begin(index, nlist, centroids, sizes)


def _ivfsq_encode_chunks(chunks, n, d, nlist, centroids, ranges, lists, nprobe, device, id_base, threshold_scan=False):
    """Rows (an iterator of (offset, fp16 rows)) -> IVF-SQ8 index: every row is encoded into the next free slot of its list."""
    return _encode_chunks(lambda sizes: _ivfsq_begin(d, nlist, centroids, ranges, sizes, device, id_base, threshold_scan), chunks, n, nlist,
                          centroids, lists, nprobe, id_base)


def build_ivfsq_index(x_f16, nlist, nprobe=16, niter=8, seed=0, device=0, id_base=0, centroids=None, ranges=None, chunk=1 << 20,
                      threshold_scan=False):
    """fp16 rows [N, d] -> HBM-resident IVF-SQ8 index (ids = id_base + row number).  `centroids` (fp16 [nlist, d]) and `ranges`
    ((vmin, vdiff), f32 [d]) can be given; by default both are trained on the rows (train_ivf_centroids, train_sq_ranges).  Lists by
    the MFMA assignment kernel, codes by the device encoder.  Shards of one index MUST share centroids and ranges.
    threshold_scan=True switches on k > 64 and range_search (Mi355xIndex.sq_threshold_scan; off by default)."""
    n, d = x_f16.shape
    if centroids is None:
        centroids = train_ivf_centroids(x_f16, nlist, niter=niter, seed=seed, device=device)
    if ranges is None:
        ranges = train_sq_ranges(x_f16, device=device, chunk=chunk)
    centroids = np.asarray(centroids).astype(np.float16)
    lists, _ = _assign_chunks(((o, x_f16[o:o + chunk]) for o in range(0, n, chunk)), n, d, nlist, centroids, device, None)
    return _ivfsq_encode_chunks(((o, x_f16[o:o + chunk]) for o in range(0, n, chunk)), n, d, nlist, centroids, ranges, lists, nprobe, device,
                                id_base, threshold_scan)


def build_ivfsq_index_from_folder(path, nlist, nprobe=16, niter=8, seed=0, device=0, centroids=None, ranges=None,
                                  max_points_per_centroid=256, chunk=1 << 20, threshold_scan=False):
    """`clip inference` output folder (img_emb_*.npy) -> IVF-SQ8 index, streaming the partitions: training on a strided sample of the
    whole folder (centroids and ranges, unless given), then one assignment pass and one encoding pass.  The result can be
    save_index()ed: the folder is self-contained (codes, not rows).  threshold_scan as in build_ivfsq_index."""
    src = path if isinstance(path, FolderRows) else FolderRows(path)
    if centroids is None or ranges is None:
        take = min(src.n, int(nlist) * int(max_points_per_centroid))
        sample = src.take(np.unique(np.linspace(0, src.n - 1, take).astype(np.int64)))
        if centroids is None:
            centroids = train_ivf_centroids(sample, nlist, niter=niter, seed=seed, device=device, max_points_per_centroid=max_points_per_centroid)
        if ranges is None:
            ranges = train_sq_ranges(sample, device=device, chunk=chunk)
    centroids = np.asarray(centroids).astype(np.float16)
    lists, _ = _assign_chunks(src.chunks(0, src.n, chunk), src.n, src.d, nlist, centroids, device, None)
    return _remember_folder(_ivfsq_encode_chunks(src.chunks(0, src.n, chunk), src.n, src.d, nlist, centroids, ranges, lists, nprobe, device, 0,
                                                 threshold_scan), src)


def build_ivfsq_index_device(fill_rows, n, d, nlist, nprobe=16, niter=8, seed=0, device=0, id_base=0, centroids=None, ranges=None,
                             chunk=1 << 20, alloc=None, points_per_centroid=64, keep_lists=False, threshold_scan=False):
    """IVF-SQ8 index over n rows PRODUCED ON THE GPU (`fill_rows(dst_ptr, row0, count, stride)` as in build_ivf_index_device, which
    must have COMPLETED when it returns): the fp16 corpus never exists whole -- a training sample (centroids and ranges, unless
    given), then per chunk one assignment pass and one encoding pass; the index keeps d bytes per row.  threshold_scan as in
    build_ivfsq_index.  Returns (index, stats dict)."""
    import time  # pylint: disable=import-outside-toplevel

    assert d % 256 == 0, "device builds take padded rows (d % 256 == 0)"
    lib = load_library()
    if alloc is None:
        def alloc(nbytes):
            import torch  # pylint: disable=import-outside-toplevel

            t = torch.empty(int(nbytes), dtype=torch.uint8, device=f"cuda:{device}")
            return t.data_ptr(), t
    t0 = time.perf_counter()
    b = IvfBuilder(d, nlist, device)
    if centroids is None or ranges is None:
        n_sample = int(min(n, nlist * points_per_centroid))
        sample_ptr, sample_keep = alloc(n_sample * d * 2)
        fill_rows(sample_ptr, 0, n_sample, max(1, n // n_sample))
        if ranges is None:
            ranges = train_sq_ranges(sample_ptr, n_sample, d, device=device)
        if centroids is None:
            train_ivf_centroids_device(b, sample_ptr, n_sample, niter=niter, seed=seed)
            centroids = np.ascontiguousarray(b.centroids())
        del sample_keep
    centroids = np.asarray(centroids).astype(np.float16)
    b.set_centroids(centroids)
    _release_cached_device_memory()
    t1 = time.perf_counter()
    lists_ptr, lists_keep = alloc(n * 4)
    rows_ptr, rows_keep = alloc(min(chunk, n) * d * 2)
    b.list_sizes(reset=True)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        fill_rows(rows_ptr, o, m, 1)
        b.assign_device(rows_ptr, m, lists_ptr + 4 * o)
    sizes = b.list_sizes()
    b.close()
    _release_cached_device_memory()
    t2 = time.perf_counter()
    index = _ivfsq_begin(d, nlist, centroids, ranges, sizes, device, id_base, threshold_scan)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        fill_rows(rows_ptr, o, m, 1)
        check(lib, lib.knnx_ivf_add_assigned_device(index._h, C.c_void_p(rows_ptr), m, id_base + o, C.c_void_p(lists_ptr + 4 * o)), "knnx")  # pylint: disable=protected-access
    index = _ivf_end(index, nlist, nprobe, centroids, id_base, n, _download_i32(lists_ptr, n, device) if keep_lists else None)
    del rows_keep, lists_keep
    _release_cached_device_memory()
    t3 = time.perf_counter()
    padded = int(((sizes + 31) // 32 * 32).sum())
    stats = {"train_s": t1 - t0, "assign_s": t2 - t1, "encode_s": t3 - t2, "list_sizes": sizes, "bytes_per_row": d + 12,
             "arena_bytes": max(padded, 32) * (d + 12)}
    return index, stats


def _save_ivfsq_index(index, folder):
    """The self-contained IVF-SQ8 folder: ivf_sq_centroids.npy (fp16 [nlist, d]), ivf_sq_vmin.npy / ivf_sq_vdiff.npy (f32 [d]),
    ivf_sq_codes.npy (u8 [n, d] in id order), ivf_sq_lists.npy (int32 [n]) and ivf_sq_manifest.json (kind "ivfsq", written last).  An
    index with the threshold scan switched on adds "threshold_scan": true (only then: other folders are byte-identical to before)."""
    import json  # pylint: disable=import-outside-toplevel

    cent = getattr(index, "ivf_centroids", None)
    if cent is None:
        raise ValueError("save_index takes an IVF-SQ8 index built by build_ivfsq_index* / load_index")
    codes, lists = index.sq_codes()
    vmin, vdiff = index.sq_quantizer()
    lo, hi = getattr(index, "ivf_row_range", (0, codes.shape[0]))
    os.makedirs(folder, exist_ok=True)
    np.save(os.path.join(folder, "ivf_sq_centroids.npy"), np.asarray(cent, dtype=np.float16))
    np.save(os.path.join(folder, "ivf_sq_vmin.npy"), vmin)
    np.save(os.path.join(folder, "ivf_sq_vdiff.npy"), vdiff)
    np.save(os.path.join(folder, "ivf_sq_codes.npy"), codes)
    np.save(os.path.join(folder, "ivf_sq_lists.npy"), lists)
    man = ivfsq_manifest(index.d, cent.shape[0], index.nprobe, (lo, hi))
    man.update(ivfsq_threshold_scan_entry(index.sq_threshold_scan))
    tmp = os.path.join(folder, IVFSQ_MANIFEST + ".part")
    with open(tmp, "w", encoding="utf-8") as f:
        json.dump(man, f, indent=1)
    os.replace(tmp, os.path.join(folder, IVFSQ_MANIFEST))
    return man


def _ivfsq_from_codes(codes, lists, lo, cent, ranges, nprobe, device, chunk=1 << 20, threshold_scan=False):
    nlist, d = cent.shape
    index = _ivfsq_begin(d, nlist, cent, ranges, np.bincount(lists, minlength=nlist).astype(np.int64), device, lo, threshold_scan)
    _add_code_chunks(index, index._lib.knnx_ivfsq_add_codes, codes, lists, lo, nlist, chunk, index._pad)  # pylint: disable=protected-access
    return _ivf_end(index, nlist, nprobe, cent, lo, codes.shape[0], np.asarray(lists, dtype=np.int32))


def _load_ivfsq_index(folder, device=0, row_range=None, devices=None):
    import json  # pylint: disable=import-outside-toplevel

    with open(os.path.join(folder, IVFSQ_MANIFEST), encoding="utf-8") as f:
        man = check_ivfsq_manifest(json.load(f), folder)
    thr_scan = read_ivfsq_threshold_scan(folder, man)
    cent = np.load(os.path.join(folder, "ivf_sq_centroids.npy"))
    ranges = (np.load(os.path.join(folder, "ivf_sq_vmin.npy")), np.load(os.path.join(folder, "ivf_sq_vdiff.npy")))
    codes = np.load(os.path.join(folder, "ivf_sq_codes.npy"), mmap_mode="r")
    lists = np.load(os.path.join(folder, "ivf_sq_lists.npy"), mmap_mode="r")
    slo, shi = man["row_range"]
    d = int(man["d"])
    if cent.shape != (man["nlist"], d) or codes.shape != (shi - slo, d) or lists.shape[0] != shi - slo or ranges[0].shape != (d,) or ranges[1].shape != (d,):
        raise ValueError(f"{folder}: the IVF-SQ8 files disagree with the manifest")
    return _split_saved_rows(lambda c, ls, lo, dev: _ivfsq_from_codes(c, ls, lo, cent, ranges, man["nprobe"], dev, threshold_scan=thr_scan),
                             codes, lists, (slo, shi), man["nprobe"], device, row_range, devices)
