"""The threshold scan of IVF-PQ on the GPU (Mi355xIndex.pq_threshold_scan; include/knnx.h: knnx_ivfpq_set_threshold_scan): range_search
and k > 64 against the numpy restatement built from the index's own centroids, codebooks and codes -- plain, behind a rotation, with a
refine store, over two shards, through save / load and through KnnHotPath.knn_search -- and the rules of the switch itself.
Indexes are built from given centroids and codebooks (no training); every shape is built once and shared by the tests of its module."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_ivfpq_gpu import NEG, _check, _data, _queries, _seed_codebooks, _small_index, np_adc_search
from test_ivfpq_refine_cpu import check_refine, np_refine_parts
from test_ivfpq_threshold_cpu import TOL, check_range, np_adc_parts

pytestmark = pytest.mark.gpu

KNNX_E_ARG, KNNX_E_STATE, KNNX_E_UNSUPPORTED = -1, -4, -5

# name -> (n, d, nlist, M, nprobe): lists of ~50 .. 225 rows, no multiple of 64 -- the smallest shapes at which the lane / tail logic,
# the share split (nprobe 1, 8, 40, 96) and the pool logic can go wrong; every M
SHAPES = {"A": (5000, 512, 96, 32, 8), "B": (5000, 768, 96, 64, 96), "C": (9000, 512, 40, 16, 40), "D": (3000, 1024, 16, 128, 1)}
_built = {}


def _shape(name):
    """(x, cent, cb, index with the switch on, codes, lists) of a shape, built once (seed d + M as in test_ivfpq_gpu.test_search_parity)."""
    if name not in _built:
        n, d, nlist, M, nprobe = SHAPES[name]
        x, cent, cb, ix = _small_index(n, d, nlist, M, nprobe, seed=d + M)
        assert ix.pq_threshold_scan is False
        ix.pq_threshold_scan = True
        assert ix.pq_threshold_scan is True
        codes, lists = ix.pq_codes()
        _built[name] = (x, cent, cb, ix, codes, lists)
    return _built[name]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for v in _built.values():
        v[3].close()
    _built.clear()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. range_search parity
@pytest.mark.parametrize("B", [1, 33, 300])
@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_range_search_parity(shape, B):
    """B = 1: min(nprobe, 128) shares per query; B = 300: two passes, 4 shares."""
    n, d, nlist, M, nprobe = SHAPES[shape]
    x, cent, cb, ix, codes, lists = _shape(shape)
    q = _queries(B, d, seed=B + 7, x=x)
    parts, amb = np_adc_parts(q, cent, cb, codes, lists, 0, nprobe)
    for thr in (0.0, 0.05, 0.1):
        lims, D, I = ix.range_search(q, thr)
        worst, band = check_range(lims, D, I, parts, amb, thr, f"{shape} B={B} thr={thr}")
        print(f"{shape} B={B} thr={thr}: {int(lims[-1])} hits, max |D - S| = {worst:.2e}, most rows within {TOL} of thr: {band}, "
              f"ambiguous probe sets {amb.mean():.2f}")


def test_range_search_protocol():
    """The two-call protocol, knnx_range_search_once with a capacity too small / large enough, lims of another threshold."""
    n, d, nlist, M, nprobe = SHAPES["A"]
    x, cent, cb, ix, codes, lists = _shape("A")
    lib, h = ix._lib, ix._h  # pylint: disable=protected-access
    q = np.ascontiguousarray(_queries(5, d, seed=3, x=x))
    thr = 0.05
    lims = np.full(6, -7, dtype=np.int64)
    assert lib.knnx_range_search(h, q.ctypes.data, 5, C.c_float(thr), lims.ctypes.data, None, None) == 0
    total = int(lims[5])
    assert lims[0] == 0 and (np.diff(lims) >= 0).all() and total > 10
    D = np.empty(total, np.float32)
    I = np.empty(total, np.int64)
    assert lib.knnx_range_search(h, q.ctypes.data, 5, C.c_float(thr), lims.ctypes.data, D.ctypes.data, I.ctypes.data) == 0
    parts, amb = np_adc_parts(q, cent, cb, codes, lists, 0, nprobe)
    check_range(lims, D, I, parts, amb, thr, "two calls")
    # _once, capacity too small: 1, lims filled, D / I untouched
    lims1 = np.zeros(6, np.int64)
    D1 = np.full(total, 123.0, np.float32)
    I1 = np.full(total, -99, np.int64)
    assert lib.knnx_range_search_once(h, q.ctypes.data, 5, C.c_float(thr), lims1.ctypes.data, D1.ctypes.data, I1.ctypes.data, total - 1) == 1
    assert np.array_equal(lims1, lims) and (D1 == 123.0).all() and (I1 == -99).all()
    # ... large enough: the same answer as the two calls, bit for bit
    assert lib.knnx_range_search_once(h, q.ctypes.data, 5, C.c_float(thr), lims1.ctypes.data, D1.ctypes.data, I1.ctypes.data, total) == 0
    assert np.array_equal(lims1, lims) and np.array_equal(I1, I) and np.array_equal(_bits(D1), _bits(D))
    # lims of another threshold
    assert lib.knnx_range_search(h, q.ctypes.data, 5, C.c_float(0.0), lims.ctypes.data, D.ctypes.data, I.ctypes.data) == KNNX_E_STATE
    assert b"lims do not match" in lib.knnx_last_error()
    # the Python wrapper (one pass, then the two calls when its guess was too small) gives the same
    l2, D2, I2 = ix.range_search(q, thr)
    assert np.array_equal(l2, lims1) and np.array_equal(I2, I1) and np.array_equal(_bits(D2), _bits(D1))


# ------------------------------------------------------------------------------------------------ 2. long lists, pool regrowth
def test_long_hit_list_takes_the_radix_sort():
    """5 000 hits of one query: more than RANGE_SORT_SMALL = 4 096."""
    n, d, nlist, M, nprobe = SHAPES["B"]
    x, cent, cb, ix, codes, lists = _shape("B")
    q = _queries(1, d, seed=11, x=x)
    lims, D, I = ix.range_search(q, -1e30)
    assert lims.tolist() == [0, n] and np.array_equal(I, np.arange(n))
    parts, _ = np_adc_parts(q, cent, cb, codes, lists, 0, nprobe)
    assert np.abs(D.astype(np.float64) - parts[0][1]).max() <= TOL


def test_pool_regrows_and_rescans():
    """256 x 9 000 hits: more than the initial 2^21-entry pool.  Every row exactly once per query."""
    n, d, nlist, M, nprobe = SHAPES["C"]
    x, cent, cb, ix, codes, lists = _shape("C")
    B = 256
    q = _queries(B, d, seed=12, x=x)
    lims, D, I = ix.range_search(q, -1e30)
    assert np.array_equal(lims, np.arange(B + 1, dtype=np.int64) * n)
    assert np.array_equal(I.reshape(B, n), np.broadcast_to(np.arange(n), (B, n)))
    cs = q.astype(np.float64) @ cent.astype(np.float32).astype(np.float64).T
    lut = np.einsum("qmt,mjt->qmj", q.astype(np.float64).reshape(B, M, d // M), cb.astype(np.float64))
    S = cs[:, lists]
    for m in range(M):
        S = S + lut[:, m, :][:, codes[:, m]]
    assert np.abs(D.reshape(B, n).astype(np.float64) - S).max() <= TOL
    # and a small request afterwards is served from the grown pool
    l2, _, I2 = ix.range_search(q[:2], 0.1)
    parts, amb = np_adc_parts(q[:2], cent, cb, codes, lists, 0, nprobe)
    for i in range(2):
        sure = parts[i][0][parts[i][1] > 0.1 + TOL]
        assert np.isin(sure, I2[l2[i]:l2[i + 1]]).all()


# ------------------------------------------------------------------------------------------------ 3. large k parity
@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_large_k_parity(shape, B):
    n, d, nlist, M, nprobe = SHAPES[shape]
    x, cent, cb, ix, codes, lists = _shape(shape)
    q = _queries(B, d, seed=B + 21, x=x)
    before = ix.pq_threshold_stats()
    for k in (65, 100, 1000, 3000, n + 10):
        D, I = ix.search(q, k)
        Do, Io, amb = np_adc_search(q, cent, cb, codes, lists, 0, nprobe, k)
        assert amb.mean() <= 0.10
        assert (Io[:, -1] == -1).all() or k < n  # k = n + 10 pads everywhere; shape D (one list) pads from k = 1 000 on
        _check(D, I, Do, Io, amb, f"{shape} B={B} k={k}")
    after = ix.pq_threshold_stats()
    assert after[0] - before[0] == 5 * B and after[1] > before[1] and after[2] - before[2] >= 5 * B
    print(f"{shape} B={B}: {(after[2] - before[2]) / (5 * B):.2f} threshold scans and {(after[3] - before[3]) / (5 * B):.0f} hits per query")


@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_large_k_two_passes(shape):
    n, d, nlist, M, nprobe = SHAPES[shape]
    x, cent, cb, ix, codes, lists = _shape(shape)
    q = _queries(300, d, seed=5, x=x)
    D, I = ix.search(q, 100)
    Do, Io, amb = np_adc_search(q, cent, cb, codes, lists, 0, nprobe, 100)
    assert amb.mean() <= 0.10
    _check(D, I, Do, Io, amb, f"{shape} B=300 k=100")


@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_large_k_bitwise(shape):
    """The first 64 of a k = 100 search are the k = 64 search, D bits and ids; a query alone and inside a batch of 33 gets the same."""
    n, d, nlist, M, nprobe = SHAPES[shape]
    x, cent, cb, ix, codes, lists = _shape(shape)
    q = _queries(33, d, seed=9, x=x)
    D64, I64 = ix.search(q, 64)
    D100, I100 = ix.search(q, 100)
    assert np.array_equal(I100[:, :64], I64) and np.array_equal(_bits(D100[:, :64]), _bits(D64))
    for i in (0, 17, 32):
        D1, I1 = ix.search(q[i:i + 1], 100)
        assert np.array_equal(I1[0], I100[i]) and np.array_equal(_bits(D1[0]), _bits(D100[i])), i


# ------------------------------------------------------------------------------------------------ 4. rotation
def test_rotated_index():
    from test_opq_gpu import _rotated_index

    n, d, nlist, M, nprobe = 3000, 512, 32, 32, 8
    x, y, A, cent, cb, ix = _rotated_index(n, d, nlist, M, nprobe, seed=5)
    ix.pq_threshold_scan = True
    codes, lists = ix.pq_codes()
    q = _queries(9, d, seed=2, x=x)
    qr = (q.astype(np.float64) @ A.astype(np.float64).T).astype(np.float32)  # the rotated-space restatement sees q' = A q
    D, I, R = ix.search_and_reconstruct(q, 100)
    Do, Io, amb = np_adc_search(qr, cent, cb, codes, lists, 0, nprobe, 100)
    assert amb.mean() <= 0.10
    _check(D, I, Do, Io, amb, "rotated k=100")
    assert (I >= 0).all()
    ids = I.reshape(-1)
    dec = cb[np.arange(M)[None, :], codes[ids]].reshape(len(ids), d).astype(np.float64)
    want = (cent[lists[ids]].astype(np.float64) + dec) @ A.astype(np.float64)  # A^T applied to the decoded rows
    assert R.shape == (9, 100, d) and np.abs(R.reshape(-1, d) - want).max() <= 1e-5
    parts, amb = np_adc_parts(qr, cent, cb, codes, lists, 0, nprobe)
    for thr in (0.0, 0.1):
        lims, Dr, Ir = ix.range_search(q, thr)
        check_range(lims, Dr, Ir, parts, amb, thr, f"rotated thr={thr}")
    ix.close()


# ------------------------------------------------------------------------------------------------ 5. refine
def test_refine_store():
    from clip_retrieval_amd import HipLibraryError
    from test_ivfpq_refine_gpu import _small_index as _refine_index

    n, d, nlist, M, nprobe = SHAPES["A"]
    x, cent, cb, ix = _refine_index(n, d, nlist, M, nprobe, seed=d + M, k_factor=8)
    codes, lists = ix.pq_codes()
    q = _queries(5, d, seed=4, x=x)
    D64, I64 = ix.search(q, 64)  # k = 64, k_factor = 8 before the switch ...
    ix.pq_threshold_scan = True
    D64b, I64b = ix.search(q, 64)  # ... and after: the k <= 64 path is untouched
    assert np.array_equal(I64, I64b) and np.array_equal(_bits(D64), _bits(D64b))
    parts, amb = np_refine_parts(q, x, cent, cb, codes, lists, 0, nprobe)
    assert amb.mean() <= 0.10
    for k, kf in ((100, 4), (1000, 8)):
        ix.k_factor = kf
        D, I = ix.search(q, k)
        worst = check_refine(D, I, parts, amb, k, k * kf, f"refine k={k} k_factor={kf}")
        print(f"refine k={k} k_factor={kf}: max |D - E| = {worst:.2e}")
    # the rows of a k = 100 search are the stored rows, bit for bit
    ix.k_factor = 4
    D, I, R = ix.search_and_reconstruct(q, 100)
    assert (I >= 0).all() and np.array_equal(_bits(R), _bits(x[I].astype(np.float32)))
    # k x k_factor > 131 072 names both numbers; k <= 64 keeps the 512 rule and its message
    ix.k_factor = 512
    with pytest.raises(HipLibraryError, match=r"code -1\).*k x k_factor = 300 x 512 exceeds 131072 candidates"):
        ix.search(q, 300)
    with pytest.raises(HipLibraryError, match=r"k x k_factor = 2 x 512 exceeds 512 candidates"):
        ix.search(q, 2)
    ix.k_factor = 4
    with pytest.raises(HipLibraryError, match=r"code -5\).*refine store"):
        ix.range_search(q, 0.1)
    ix.close()


# ------------------------------------------------------------------------------------------------ 6. the switch
def test_switch_semantics():
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import Mi355xIndex, build_ivf_index, build_ivfpq_index

    x, cent, cb, ix = _small_index(1000, 512, 8, 16, 2, seed=1)
    q = _queries(2, 512, 1, x)

    def refused():
        with pytest.raises(HipLibraryError, match=r"code -5\): k > 64 is not supported on an IVF-PQ index$"):
            ix.search(q, 65)
        with pytest.raises(HipLibraryError, match=r"code -5\): range_search is not supported on an IVF-PQ index$"):
            ix.range_search(q, 0.5)

    assert ix.pq_threshold_scan is False
    refused()  # a default-built index answers as it always has
    D40, I40 = ix.search(q, 40)
    ix.pq_threshold_scan = True
    D, I = ix.search(q, 65)
    assert np.array_equal(I[:, :40], I40) and np.array_equal(_bits(D[:, :40]), _bits(D40))
    lims, _, _ = ix.range_search(q, 0.0)
    assert lims[-1] > 0
    ix.pq_threshold_scan = False
    assert ix.pq_threshold_scan is False
    refused()
    D40b, I40b = ix.search(q, 40)
    assert np.array_equal(I40b, I40) and np.array_equal(_bits(D40b), _bits(D40))
    ix.close()
    # built switched on
    on = build_ivfpq_index(x, 8, 16, nprobe=2, centroids=cent, codebooks=cb, threshold_scan=True)
    assert on.pq_threshold_scan is True
    assert np.array_equal(on.search(q, 65)[1], I)
    on.close()
    # not an IVF-PQ index: the getter says False, the setter is an error
    flat = Mi355xIndex(512)
    flat.add(x)
    ivf = build_ivf_index(x, 8, nprobe=2, centroids=cent)
    for other in (flat, ivf):
        assert other.pq_threshold_scan is False
        with pytest.raises(HipLibraryError, match=r"code -4\).*not an IVF-PQ index"):
            other.pq_threshold_scan = True
        assert other.search(q, 65)[1].shape == (2, 65)  # and they serve large k as before
        other.close()


# ------------------------------------------------------------------------------------------------ 7. shards
def test_two_shards_on_one_gpu():
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import ShardedMi355xIndex, build_ivfpq_index

    n, d, nlist, M, nprobe = SHAPES["A"]
    x, cent, cb, single, codes, lists = _shape("A")
    cut = [0, 2500, n]
    shards = [build_ivfpq_index(x[cut[g]:cut[g + 1]], nlist, M, nprobe=nprobe, id_base=cut[g], centroids=cent, codebooks=cb) for g in range(2)]
    ix = ShardedMi355xIndex.from_shards(shards, cut[:2])
    q = _queries(7, d, seed=6, x=x)
    assert ix.pq_threshold_scan is False
    with pytest.raises(HipLibraryError, match="k > 64 is not supported on an IVF-PQ index"):
        ix.search(q, 100)
    ix.pq_threshold_scan = True  # sets every shard; the adopted Mi355xIndex objects gave their handles up, so ask the shards themselves
    lib, h = ix._lib, ix._h  # pylint: disable=protected-access
    assert ix.pq_threshold_scan is True and ix.nshards == 2
    assert all(lib.knnx_ivfpq_threshold_scan(C.c_void_p(lib.knnx_shards_get(h, g))) == 1 for g in range(2))
    D, I = ix.search(q, 100)
    D1, I1 = single.search(q, 100)
    assert np.array_equal(I, I1) and np.abs(D - D1).max() <= 1e-6
    lims, Dr, Ir = ix.range_search(q, 0.05)
    l1, Dr1, Ir1 = single.range_search(q, 0.05)
    assert np.array_equal(lims, l1) and np.array_equal(Ir, Ir1) and np.abs(Dr - Dr1).max() <= 1e-6
    ix.close()


# ------------------------------------------------------------------------------------------------ 8. saved form, service
def test_save_load_keeps_the_switch(tmp_path):
    from clip_retrieval_amd import HipLibraryError, knn

    n, d, nlist, M, nprobe = SHAPES["A"]
    x, cent, cb, ix, codes, lists = _shape("A")
    q = _queries(3, d, seed=8, x=x)
    D0, I0 = ix.search(q, 100)
    out = str(tmp_path / "on")
    man = knn.save_index(ix, out)
    assert man["threshold_scan"] is True
    with open(os.path.join(out, knn.IVFPQ_MANIFEST), encoding="utf-8") as f:
        assert json.load(f)["threshold_scan"] is True
    loaded = knn.load_index(out)
    assert loaded.pq_threshold_scan is True
    D1, I1 = loaded.search(q, 100)
    assert np.array_equal(I0, I1) and np.array_equal(_bits(D0), _bits(D1))
    loaded.close()
    sharded = knn.load_index(out, devices=[0, 0])
    assert sharded.pq_threshold_scan is True
    assert np.array_equal(sharded.search(q, 100)[1], I0)
    sharded.close()
    # a manifest without the key (every folder written before the switch existed) loads with it off
    with open(os.path.join(out, knn.IVFPQ_MANIFEST), encoding="utf-8") as f:
        m = json.load(f)
    del m["threshold_scan"]
    with open(os.path.join(out, knn.IVFPQ_MANIFEST), "w", encoding="utf-8") as f:
        json.dump(m, f)
    off = knn.load_index(out)
    assert off.pq_threshold_scan is False
    with pytest.raises(HipLibraryError, match="k > 64 is not supported on an IVF-PQ index"):
        off.search(q, 100)
    # ... and an index saved with the switch off writes no key
    assert "threshold_scan" not in knn.save_index(off, str(tmp_path / "off"))
    off.close()


def _np_dedup_keep(vecs, thr=0.94):
    """clip_back.py:290-309 restated: ranks kept after the connected components of {normalised inner product > thr}: the smallest rank
    of every component."""
    v = vecs.astype(np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    n = len(v)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j in zip(*np.nonzero(np.triu(v @ v.T > thr, 1))):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([i for i in range(n) if find(i) == i], dtype=np.int64)


def test_service_serves_the_reference_request_sizes():
    """KnnHotPath.knn_search with num_result_ids = 100 and 3 000 (deduplicate=True) and the >= 100 000 request of the probe-widening
    branch, on a switched-on IVF-PQ index.  Order: the ids are compared as the restatement ranks them, except that neighbours whose
    float64 scores lie within 1e-5 of each other may swap (the tolerance of _check)."""
    from types import SimpleNamespace

    from clip_retrieval_amd.service import KnnHotPath

    n, d, nlist, M, nprobe = SHAPES["A"]
    x, cent, cb, ix, codes, lists = _shape("A")
    res = SimpleNamespace(image_index=ix, text_index=ix, metadata_is_ordered_by_ivf=False, safety_model=None, violence_detector=None)
    hp = KnnHotPath()
    q = _queries(1, d, seed=14, x=x)
    parts, amb = np_adc_parts(q, cent, cb, codes, lists, 0, nprobe)
    assert not amb[0]
    ids, S = parts[0]
    order = np.lexsort((ids, -S))
    for k in (100, 3000):
        dist, ind = hp.knn_search(q, "image", k, res, True, False, False)
        top = order[:k]
        dec = cent[lists[ids[top]]].astype(np.float32) + cb[np.arange(M)[None, :], codes[ids[top]]].reshape(len(top), d)
        want = ids[top][_np_dedup_keep(dec)]
        got = np.asarray(ind, dtype=np.int64)
        assert len(got) == len(want) and set(got.tolist()) == set(want.tolist()), f"k={k}"
        where = {int(a): j for j, a in enumerate(ids)}
        sg = np.array([S[where[int(a)]] for a in got])
        assert (np.diff(sg) <= 1e-5).all() and np.abs(np.asarray(dist, dtype=np.float64) - sg).max() <= 1e-5, f"k={k}"
        swapped = np.flatnonzero(got != want)
        assert all(abs(S[where[int(got[j])]] - S[where[int(want[j])]]) <= 1e-5 for j in swapped), f"k={k}"
    # >= 100 000: nprobe widened to ceil(1e5 / 3000) = 34 of 96 lists for the request and put back
    dist, ind = hp.knn_search(q, "image", 100000, res, False, False, False)
    assert ix.nprobe == nprobe
    wide, _ = np_adc_parts(q, cent, cb, codes, lists, 0, 34)
    assert sorted(int(i) for i in ind) == wide[0][0].tolist()
    # ... and with every list probed: all 5 000 rows, once
    ix.nprobe = nlist
    try:
        dist, ind = hp.knn_search(q, "image", 100000, res, False, False, False)
    finally:
        ix.nprobe = nprobe
    assert sorted(int(i) for i in ind) == list(range(n)) and (np.diff(np.asarray(dist)) <= 0).all()
