"""faiss-`Index`-shaped object over the MI355X kNN library (search half of the hot path).

Mirrors exactly the part of the faiss Index API the reference exercises:
  * `search_and_reconstruct(x, k) -> (D, I, R)`   clip_retrieval/clip_back.py:362
  * `search(x, k) -> (D, I)`                      clip_retrieval/clip_filter.py:55
  * `range_search(x, thresh) -> (lims, D, I)`     clip_retrieval/clip_filter.py:52, clip_back.py:294
  * `.ntotal`, `.d`, `add(x)`, `reconstruct(i)`   ivf_metadata_ordering.py:51, clip_back.py:292-293
so an instance can be dropped into `ClipResource.image_index` / `.text_index` (clip_back.py:781-782).

Same argument meaning and error behaviour as faiss: float32 C-contiguous [n, d] queries (anything else
raises like faiss' SWIG wrapper does), int64 labels, -1 / -FLT_MAX padding, exceptions on misuse.
Thread-safe: clip_back serves each request on its own werkzeug thread with n=1 (clip_back.py:1018);
concurrent callers are coalesced into one HBM scan of up to 256 queries (_SCAN_QUERIES) by a leader/follower batcher.

First of the kNN modules (knn_index <- knn_train <- knn_build <- knn_store; knn.py is the public face): imports none of the others.
"""

import ctypes as C
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


def _pad_rotation(A, dpad):
    """[d, d] -> [dpad, dpad]: the zero pad columns of the rows map onto themselves."""
    A = np.asarray(A, dtype=np.float32)
    d = A.shape[0]
    if d == dpad:
        return np.ascontiguousarray(A)
    out = np.eye(dpad, dtype=np.float32)
    out[:d, :d] = A
    return out


class _FaissShaped:
    """The part of the faiss Index surface clip_back / clip_filter exercise, on top of `range_search`, `ntotal` and the three library
    entry points the concrete index (one GPU or row-sharded) names: _SEARCH, _RECONSTRUCT and _ID_ORDER."""

    _SEARCH = _RECONSTRUCT = _ID_ORDER = None

    def _search_raw(self, q, k, want_r):
        n = q.shape[0]
        qp = np.ascontiguousarray(self._pad(q))
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        R = np.empty((n, k, self._dpad), dtype=np.float32) if want_r else None
        check(self._lib, getattr(self._lib, self._SEARCH)(self._h, qp.ctypes.data, n, int(k), D.ctypes.data, I.ctypes.data,
                                                          R.ctypes.data if want_r else None), "knnx")
        if want_r and self._dpad != self.d:
            R = np.ascontiguousarray(R[:, :, : self.d])
        return D, I, R

    def reconstruct_batch(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        out = np.empty((keys.shape[0], self._dpad), dtype=np.float32)
        check(self._lib, getattr(self._lib, self._RECONSTRUCT)(self._h, keys.ctypes.data, keys.shape[0], out.ctypes.data), "knnx")
        return np.ascontiguousarray(out[:, : self.d])

    def _id_order(self, new_to_old):
        out = np.empty(self.ntotal, dtype=np.int64)
        check(self._lib, getattr(self._lib, self._ID_ORDER)(self._h, *((None, out.ctypes.data) if new_to_old else (out.ctypes.data, None))), "knnx")
        return out

    def ivf_old_to_new(self):
        """int64 [ntotal]: old_to_new[i] = id_base + the list-ordered ordinal of the row with id id_base + i (include/knnx.h,
        "List-ordered ids"); with id_base = 0 the array of the reference's get_old_to_new_mapping (ivf_metadata_ordering.py:46-64).
        Sharded: the concatenation of the shards' arrays (each list-sorted inside its own row range), a permutation of [0, ntotal)."""
        return self._id_order(False)

    def ivf_new_to_old(self):
        """int64 [ntotal]: the ids of the lists one after the other, list 0 first -- row o of a list-ordered metadata store is the
        source row new_to_old[o] - id_base.  Sharded: the concatenation of the shards' arrays."""
        return self._id_order(True)

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

    _SEARCH, _RECONSTRUCT, _ID_ORDER = "knnx_search", "knnx_reconstruct", "knnx_ivf_id_order"

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
        self._forget_folder()  # the rows no longer come from one folder
        return self._grown(n_before, lists)

    def _forget_folder(self):
        """Drop what bound the index to the embeddings folder it was built from."""
        for name in ("ivf_source", "embeddings_folder", "ivf_folder", "ivf_folder_files"):
            if hasattr(self, name):
                delattr(self, name)

    # ------------------------------------------------------------------ shrinking a built IVF index (include/knnx.h)
    def _shrunk(self, kept, base):
        """After rows were removed (kept: the old ids of the survivors in new-id order): ivf_lists / ivf_row_range follow where the index
        carries them, and what bound the index to the folder it was built from is dropped -- the folder's rows no longer are its rows."""
        if getattr(self, "ivf_lists", None) is not None:
            self.ivf_lists = np.ascontiguousarray(np.asarray(self.ivf_lists, dtype=np.int32)[kept - base])
        if getattr(self, "ivf_row_range", None) is not None:
            self.ivf_row_range = (self.ivf_row_range[0], self.ivf_row_range[0] + len(kept))
        self._forget_folder()

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

    # ------------------------------------------------------------------ searching (search, reconstruct_batch: _FaissShaped)
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

    _SEARCH, _RECONSTRUCT, _ID_ORDER = "knnx_shards_search", "knnx_shards_reconstruct", "knnx_shards_id_order"

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
