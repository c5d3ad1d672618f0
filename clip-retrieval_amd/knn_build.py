"""The builders of the IVF indexes -- {IVF-Flat, IVF-PQ, IVF-SQ8} x {host array, embeddings folder, rows produced on the GPU} -- over
two drivers: _build_from_chunks (host rows: an assignment pass, then knnx_ivf_begin / add_assigned / end) and _build_on_device (rows
produced on the GPU, with the scratch choreography BASELINE config 5 depends on).  Each kind adds how its quantiser is trained and its
_ivf*_begin.  Third of the kNN modules (knn_index <- knn_train <- knn_build <- knn_store)."""

import ctypes as C
import glob
import os
import time

import numpy as np

from ._lib import HipLibraryError, check, load_library
from .knn_index import Mi355xIndex, _pad_rotation
from .knn_train import (OPQ_SAMPLE_ROWS, PQ_SAMPLE_ROWS, IvfBuilder, PqBuilder, _check_opq_dim, _resolve_rotation, _rotation_out_dim,
                        opq_embedding, rotate_rows, rotate_rows_device, train_ivf_centroids, train_ivf_centroids_device, train_ivfpq,
                        train_opq_device, train_pq_codebooks, train_sq_ranges)


def embedding_files(folder):
    """The `img_emb_*.npy` / `text_emb_*.npy` files of one `clip inference` output folder, in partition
    order (zero-padded names sort correctly: writer.py:22,67)."""
    # (not the sidecars save_index() writes -- ivf_centroids.npy / ivf_lists.npy: an index saved INTO its embeddings folder must not
    # turn into two more partitions at the next load)
    files = sorted(f for f in glob.glob(os.path.join(folder, "*.npy")) if not os.path.basename(f).startswith("ivf_"))
    if not files:
        raise ValueError(f"no .npy embedding files under {folder}")
    return files


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


def _ivf_end(index, nlist, nprobe, centroids, id_base, n, lists=None):
    """knnx_ivf_end, then what every built IVF index carries: nprobe, its centroids and row range, the lists where they are known.
    centroids None: neither they nor the row range are recorded (build_ivf_index_device never did)."""
    check(index._lib, index._lib.knnx_ivf_end(index._h), "knnx")  # pylint: disable=protected-access
    index.nprobe = min(int(nprobe), nlist)
    if centroids is not None:
        index.ivf_centroids, index.ivf_row_range = np.asarray(centroids, dtype=np.float16), (int(id_base), int(id_base) + int(n))
    if lists is not None:
        index.ivf_lists = lists
    return index


def _encode_chunks(begin, chunks, n, nlist, centroids, lists, nprobe, id_base):
    """Rows (an iterator of (offset, fp16 rows)) -> a compressed IVF index: begin(list sizes) makes the index and opens the build."""
    index = begin(_list_sizes(lists, nlist))
    _add_assigned_chunks(index, chunks, lists, nlist, id_base)
    return _ivf_end(index, nlist, nprobe, centroids, id_base, n, lists)


def _assign_chunks(chunks, n, d, nlist, centroids, device, A):
    """List of every row (rotated by A first when there is one) -> (lists int32 [n], seconds spent rotating).  The offsets of the
    chunks index `lists`: a shard that starts at row lo hands over (offset - lo, rows)."""
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


def _array_chunks(x, chunk):
    """chunks() of a host array (or memmap): every call streams it once as (offset, rows)."""
    return lambda: ((o, x[o:o + chunk]) for o in range(0, x.shape[0], chunk))


def _folder_sample(src, take):
    """The training sample of a folder: <= take rows at even strides over the WHOLE folder, so that every shard trains the same."""
    return src.take(np.unique(np.linspace(0, src.n - 1, take).astype(np.int64)))


def _ivfflat_from_chunks(chunks, n, d, nlist, centroids, nprobe, device, id_base, lists=None):
    """Host rows -> IVF-Flat index; chunks() gives an iterator of (offset, fp16 rows) and is called once per pass: the assignment
    pass (skipped when a saved index names the `lists`), then the scatter into the list-sorted arena."""
    if lists is None:
        lists = _assign_chunks(chunks(), n, d, nlist, centroids, device, None)[0]
    # (the lists are kept for tests / recall measurement, and for save_index(index, folder, embeddings_folder=...))
    return _encode_chunks(lambda sizes: _ivf_begin(Mi355xIndex(d, device=device, id_base=id_base), nlist, centroids, sizes), chunks(), n, nlist,
                          centroids, lists, nprobe, id_base)


def _scatter_into_ivf(src, lo, hi, centroids, lists, nprobe, device, chunk):
    """Rows [lo, hi) of `src` into a list-sorted arena on `device` (ids = global row numbers).  Given every row's list id (load_index)
    it streams the rows once: no training, no assignment; lists None: the assignment pass comes first."""
    index = _ivfflat_from_chunks(lambda: ((o - lo, x) for o, x in src.chunks(lo, hi, chunk)), hi - lo, src.d, centroids.shape[0], centroids,
                                 nprobe, device, lo, lists)
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


def _torch_alloc(device):
    """The default `alloc` of the device builders: torch uint8 tensors (torch is this package's device-memory plumbing)."""
    def alloc(nbytes):
        import torch  # pylint: disable=import-outside-toplevel

        t = torch.empty(int(nbytes), dtype=torch.uint8, device=f"cuda:{device}")
        return t.data_ptr(), t
    return alloc


def _device_sample(alloc, fill_rows, n, count, d):
    """`count` rows at even strides over the n rows, generated into a scratch buffer of their own -> (pointer, keep-alive object)."""
    ptr, keep = alloc(count * d * 2)
    fill_rows(ptr, 0, count, max(1, n // count))
    return ptr, keep


def _build_on_device(train, fill_rows, n, d, nlist, nprobe, device, id_base, chunk, alloc, keep_lists=False, record=True,
                     release_after_assign=True):
    """What the three build_*_index_device share.  train(alloc) -> (the IvfBuilder holding the centroids, the rotation A or None, the
    centroids, begin) does what is the kind's own: it trains its quantiser from samples it generates (_device_sample) and frees, and
    begin(list sizes) makes the index and opens the build (_ivf*_begin).  Returns (index, list sizes, (train_s, assign_s, seconds of
    the scatter / encode pass, seconds spent rotating in the assignment pass)).

    The order of scratch allocations, fills and frees below is behaviour, not style -- whether BASELINE config 5 (256 GB of rows on one
    card) fits depends on it, and tests/test_build_trace_gpu.py pins it: the samples are gone before the list and row buffers come, the
    rotated chunk and the IvfBuilder before the arena does (begin), and a chunk is handed to the index once, never held twice."""
    assert d % 256 == 0, "device builds take padded rows (d % 256 == 0)"
    lib = load_library()
    alloc = alloc or _torch_alloc(device)
    t0 = time.perf_counter()
    b, A, centroids, begin = train(alloc)
    _release_cached_device_memory()  # the arena allocated below needs the bytes a caching allocator would sit on
    t1 = time.perf_counter()
    # pass 1: list of every row (4 bytes per row stay on the device), list sizes
    lists_ptr, lists_keep = alloc(n * 4)
    rows_ptr, rows_keep = alloc(min(chunk, n) * d * 2)
    rot_ptr, rot_keep = alloc(min(chunk, n) * _rotation_out_dim(A, d) * 2) if A is not None else (rows_ptr, None)
    rotate_s = 0.0
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
    if release_after_assign:
        _release_cached_device_memory()
    t2 = time.perf_counter()
    # pass 2: every chunk again, into the list-sorted arena (an IVF-PQ / IVF-SQ8 index rotates and encodes it there)
    index = begin(sizes)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        fill_rows(rows_ptr, o, m, 1)
        check(lib, lib.knnx_ivf_add_assigned_device(index._h, C.c_void_p(rows_ptr), m, id_base + o, C.c_void_p(lists_ptr + 4 * o)), "knnx")  # pylint: disable=protected-access
    # (keep_lists -- tests / recall measurements: the list of every row, 4 bytes per row to the host)
    _ivf_end(index, nlist, nprobe, centroids if record else None, id_base, n, _download_i32(lists_ptr, n, device) if keep_lists else None)
    del rows_keep, lists_keep
    _release_cached_device_memory()
    return index, sizes, (t1 - t0, t2 - t1, time.perf_counter() - t2, rotate_s)


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
    n_sample = int(min(n, nlist * points_per_centroid)) if sample_rows is None else int(sample_rows)

    def train(alloc):
        b = IvfBuilder(d, nlist, device)
        sample_ptr, sample_keep = _device_sample(alloc, fill_rows, n, n_sample, d)
        train_ivf_centroids_device(b, sample_ptr, n_sample, niter=niter, seed=seed)
        cent = np.ascontiguousarray(b.centroids())
        del sample_keep
        return b, None, cent, lambda sizes: _ivf_begin(Mi355xIndex(d, device=device, id_base=id_base), nlist, cent, sizes)

    # (this builder never recorded ivf_centroids / ivf_row_range on its index, and still does not)
    index, sizes, clock = _build_on_device(train, fill_rows, n, d, nlist, nprobe, device, id_base, chunk, alloc, keep_lists, record=False)
    return index, {"train_s": clock[0], "assign_s": clock[1], "scatter_s": clock[2], "n_sample": n_sample, "list_sizes": sizes}


def build_ivf_index(x_f16, nlist, nprobe=16, niter=8, seed=0, device=0, id_base=0, centroids=None, chunk=1 << 20):
    """fp16 rows [N, d] -> HBM-resident IVF-Flat index (ids = id_base + row number, like the flat index).  `x_f16` may be a
    numpy memmap: rows are streamed twice in chunks (assignment, then scatter into the list-sorted arena)."""
    n, d = x_f16.shape
    if centroids is None:
        centroids = train_ivf_centroids(x_f16, nlist, niter=niter, seed=seed, device=device)
    return _ivfflat_from_chunks(_array_chunks(x_f16, chunk), n, d, nlist, np.asarray(centroids).astype(np.float16), nprobe, device, id_base)


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
        sample = _folder_sample(src, min(src.n, int(nlist) * int(max_points_per_centroid)))
        centroids = train_ivf_centroids(sample, nlist, niter=niter, seed=seed, device=device, max_points_per_centroid=max_points_per_centroid)
    return _scatter_into_ivf(src, lo, hi, np.asarray(centroids).astype(np.float16), None, nprobe, device, chunk)


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


def _ivfpq_from_chunks(chunks, n, d, nlist, M, centroids, codebooks, nprobe, device, id_base, rotation, refine, k_factor, threshold_scan):
    """Host rows -> IVF-PQ index; chunks() gives an iterator of (offset, fp16 rows) and is called once per pass: the assignment pass
    (of the rotated rows when there is a rotation), then the encoding pass."""
    centroids = np.asarray(centroids).astype(np.float16)
    lists, rotate_s = _assign_chunks(chunks(), n, d, nlist, centroids, device, rotation)
    index = _ivfpq_encode_chunks(chunks(), n, d, nlist, M, centroids, codebooks, lists, nprobe, device, id_base, rotation, refine, k_factor,
                                 threshold_scan)
    index.rotate_s = rotate_s
    return index


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
    return _ivfpq_from_chunks(_array_chunks(x_f16, chunk), n, d, nlist, M, centroids, codebooks, nprobe, device, id_base, A, refine, k_factor,
                              threshold_scan)


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
        sample = _folder_sample(src, min(src.n, max(int(nlist) * int(max_points_per_centroid), PQ_SAMPLE_ROWS)))
        A, _ = _resolve_rotation(sample, M, opq, A, seed, device, opq_dim)
        if centroids is None or codebooks is None:
            centroids, codebooks = train_ivfpq(sample, nlist, M, niter=niter, pq_niter=pq_niter, seed=seed, device=device,
                                               centroids=centroids, max_points_per_centroid=max_points_per_centroid, rotation=A)[:2]
    index = _ivfpq_from_chunks(lambda: src.chunks(0, src.n, chunk), src.n, src.d, nlist, M, centroids, codebooks, nprobe, device, 0, A, refine,
                               k_factor, threshold_scan)
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
    opq_s = [0.0]

    def train(alloc):
        t0 = time.perf_counter()
        A = None if rotation is None else _resolve_rotation(None, M, opq, rotation, seed, device, opq_dim)[0]
        if A is not None and A.shape[0] == A.shape[1]:
            A = _pad_rotation(A, d)
        if opq_dim is not None and A is None and not opq:
            raise ValueError("opq_dim needs opq=True or rotation=")
        if A is None and opq:
            n_os = int(min(n, opq_sample_rows))
            os_ptr, os_keep = _device_sample(alloc, fill_rows, n, n_os, d)
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
            opq_s[0] = time.perf_counter() - t0
        dq = _rotation_out_dim(A, d)  # the width behind the rotation: training samples, centroids, codebooks, the rotated chunk

        def rotated(ptr, count):  # -> (pointer to the rotated rows, their owner): a second buffer, or the rows themselves without a rotation
            if A is None:
                return ptr, None
            rp, rk = alloc(count * dq * 2)
            rotate_rows_device(A, ptr, count, rp, device)
            return rp, rk

        b = IvfBuilder(dq, nlist, device)
        cent, cb = centroids, codebooks
        if cent is None:
            n_sample = int(min(n, nlist * points_per_centroid))
            sample_ptr, sample_keep = _device_sample(alloc, fill_rows, n, n_sample, d)
            sample_ptr, sample_rot_keep = rotated(sample_ptr, n_sample)
            train_ivf_centroids_device(b, sample_ptr, n_sample, niter=niter, seed=seed)
            cent = np.ascontiguousarray(b.centroids())
            del sample_keep, sample_rot_keep
        cent = np.asarray(cent).astype(np.float16)
        b.set_centroids(cent)
        if cb is None:
            n_ps = int(min(n, pq_sample_rows))
            ps_ptr, ps_keep = alloc(n_ps * d * 2)
            pl_ptr, pl_keep = alloc(n_ps * 4)
            fill_rows(ps_ptr, 0, n_ps, max(1, n // n_ps))
            ps_ptr, ps_rot_keep = rotated(ps_ptr, n_ps)
            b.assign_device(ps_ptr, n_ps, pl_ptr)
            pb = PqBuilder(dq, M, device)
            pb.set_sample_device(ps_ptr, pl_ptr, n_ps, cent)
            cb = train_pq_codebooks(pb, niter=pq_niter, seed=seed)
            pb.close()
            del ps_keep, ps_rot_keep, pl_keep
        return b, A, cent, lambda sizes: _ivfpq_begin(d, nlist, M, cent, cb, sizes, device, id_base, A, refine, k_factor, threshold_scan)

    # (release_after_assign=False: this builder has never emptied the allocator's cache between the rotated chunk and the arena)
    index, sizes, clock = _build_on_device(train, fill_rows, n, d, nlist, nprobe, device, id_base, chunk, alloc, release_after_assign=False)
    code_bytes, row_bytes = index.pq_arena_bytes()
    return index, {"train_s": clock[0], "assign_s": clock[1], "encode_s": clock[2], "list_sizes": sizes,
                   "bytes_per_row": M + 12 + (2 * d if refine else 0), "rotate_s": clock[3], "opq_s": opq_s[0],
                   "code_arena_bytes": code_bytes, "row_arena_bytes": row_bytes}


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


def _ivfsq_from_chunks(chunks, n, d, nlist, centroids, ranges, nprobe, device, id_base, threshold_scan):
    """Host rows -> IVF-SQ8 index; chunks() gives an iterator of (offset, fp16 rows) and is called once per pass: assignment, encoding."""
    centroids = np.asarray(centroids).astype(np.float16)
    lists = _assign_chunks(chunks(), n, d, nlist, centroids, device, None)[0]
    return _ivfsq_encode_chunks(chunks(), n, d, nlist, centroids, ranges, lists, nprobe, device, id_base, threshold_scan)


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
    return _ivfsq_from_chunks(_array_chunks(x_f16, chunk), n, d, nlist, centroids, ranges, nprobe, device, id_base, threshold_scan)


def build_ivfsq_index_from_folder(path, nlist, nprobe=16, niter=8, seed=0, device=0, centroids=None, ranges=None,
                                  max_points_per_centroid=256, chunk=1 << 20, threshold_scan=False):
    """`clip inference` output folder (img_emb_*.npy) -> IVF-SQ8 index, streaming the partitions: training on a strided sample of the
    whole folder (centroids and ranges, unless given), then one assignment pass and one encoding pass.  The result can be
    save_index()ed: the folder is self-contained (codes, not rows).  threshold_scan as in build_ivfsq_index."""
    src = path if isinstance(path, FolderRows) else FolderRows(path)
    if centroids is None or ranges is None:
        sample = _folder_sample(src, min(src.n, int(nlist) * int(max_points_per_centroid)))
        if centroids is None:
            centroids = train_ivf_centroids(sample, nlist, niter=niter, seed=seed, device=device, max_points_per_centroid=max_points_per_centroid)
        if ranges is None:
            ranges = train_sq_ranges(sample, device=device, chunk=chunk)
    return _remember_folder(_ivfsq_from_chunks(lambda: src.chunks(0, src.n, chunk), src.n, src.d, nlist, centroids, ranges, nprobe, device, 0,
                                               threshold_scan), src)


def build_ivfsq_index_device(fill_rows, n, d, nlist, nprobe=16, niter=8, seed=0, device=0, id_base=0, centroids=None, ranges=None,
                             chunk=1 << 20, alloc=None, points_per_centroid=64, keep_lists=False, threshold_scan=False):
    """IVF-SQ8 index over n rows PRODUCED ON THE GPU (`fill_rows(dst_ptr, row0, count, stride)` as in build_ivf_index_device, which
    must have COMPLETED when it returns): the fp16 corpus never exists whole -- a training sample (centroids and ranges, unless
    given), then per chunk one assignment pass and one encoding pass; the index keeps d bytes per row.  threshold_scan as in
    build_ivfsq_index.  Returns (index, stats dict)."""
    def train(alloc):
        b = IvfBuilder(d, nlist, device)
        cent, rng = centroids, ranges
        if cent is None or rng is None:
            n_sample = int(min(n, nlist * points_per_centroid))
            sample_ptr, sample_keep = _device_sample(alloc, fill_rows, n, n_sample, d)
            if rng is None:
                rng = train_sq_ranges(sample_ptr, n_sample, d, device=device)
            if cent is None:
                train_ivf_centroids_device(b, sample_ptr, n_sample, niter=niter, seed=seed)
                cent = np.ascontiguousarray(b.centroids())
            del sample_keep
        cent = np.asarray(cent).astype(np.float16)
        b.set_centroids(cent)
        return b, None, cent, lambda sizes: _ivfsq_begin(d, nlist, cent, rng, sizes, device, id_base, threshold_scan)

    index, sizes, clock = _build_on_device(train, fill_rows, n, d, nlist, nprobe, device, id_base, chunk, alloc, keep_lists)
    padded = int(((sizes + 31) // 32 * 32).sum())
    return index, {"train_s": clock[0], "assign_s": clock[1], "encode_s": clock[2], "list_sizes": sizes, "bytes_per_row": d + 12,
                   "arena_bytes": max(padded, 32) * (d + 12)}
