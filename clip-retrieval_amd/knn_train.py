"""The device trainers of the IVF indexes: coarse k-means (IvfBuilder), PQ codebooks (PqBuilder), the OPQ rotation and the SQ8 ranges,
the rotation helpers, the synthetic corpus generator and the parsers of faiss index-factory strings.  Second of the kNN modules
(knn_index <- knn_train <- knn_build <- knn_store): it makes no index, so it imports only a padding helper from knn_index."""

import ctypes as C

import numpy as np

from ._lib import check, load_library
from .knn_index import _pad_rotation


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


# ------------------------------------------------------------------------------------------------------------
# IVF-PQ (faiss IndexIVFPQ(IndexFlatIP(d), d, nlist, M, 8), METRIC_INNER_PRODUCT, by_residual): what autofaiss builds for large
# corpora (clip_index.py:12-66; the reference notebook's OPQ256_768,IVF16384_HNSW32,PQ256x8 without HNSW; OPQ: train_opq below).  The coarse
# quantiser is the IVF-Flat one; every row is kept as M code bytes (csrc/knn_pq_kernels.hip), so 1 B x 768 fits one GPU.
# ------------------------------------------------------------------------------------------------------------
PQ_SAMPLE_ROWS = 256 * 256  # rows of the codebook training sample (faiss: 256 x ksub)


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
