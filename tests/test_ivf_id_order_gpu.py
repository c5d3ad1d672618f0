"""List-ordered ids (reorder_metadata_by_ivf_index) on the GPU: the export and the translation kernels against the numpy restatement on
crafted IVF-Flat lists (both sides of a tile, empty lists in a row and at both ends), on IVF-PQ indexes of every kind, over two shards,
under concurrent searches, through KnnHotPath with a re-ordered Arrow folder, and across save / load."""
import ctypes as C
import os
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from test_ivf_id_order_cpu import np_id_order, np_map_ids, write_arrow_folder
from test_ivfpq_gpu import _data, _queries, _seed_codebooks

pytestmark = pytest.mark.gpu

D = 256
SIZES = np.asarray([0, 1, 31, 32, 33, 0, 0, 65, 0], dtype=np.int64)  # 162 rows
E_ARG, E_STATE = "code -1)", "code -4)"


def _crafted(id_base, seed=0):
    """IVF-Flat index over the crafted lists through set_ivf_lists -> (index, ids in arena order)."""
    from clip_retrieval_amd.knn import Mi355xIndex

    n = int(SIZES.sum())
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n).astype(np.int64) + id_base
    ix = Mi355xIndex(D, id_base=id_base)
    ix.add(_data(n, D, seed + 1))
    ix.set_ivf_lists(_data(len(SIZES), D, seed + 2), SIZES, ids)
    return ix, ids


def _check_mapping(ix, new_to_old, id_base):
    n = len(new_to_old)
    want_o2n, want_n2o = np_id_order([new_to_old], id_base)
    got_n2o, got_o2n = ix.ivf_new_to_old(), ix.ivf_old_to_new()
    assert got_n2o.dtype == np.int64 and got_o2n.dtype == np.int64 and got_n2o.shape == (n,) and got_o2n.shape == (n,)
    assert np.array_equal(got_n2o, want_n2o)
    assert np.array_equal(got_o2n, want_o2n)
    inverse = np.empty(n, dtype=np.int64)
    inverse[new_to_old - id_base] = np.arange(n)
    assert np.array_equal(got_o2n, inverse + id_base)
    assert np.array_equal(np.sort(got_o2n), np.arange(n) + id_base)  # a permutation
    return got_o2n


@pytest.mark.parametrize("chunk", [None, "64"])
@pytest.mark.parametrize("id_base", [0, 1000])
def test_crafted_lists_through_set_ivf_lists(id_base, chunk, monkeypatch):
    """new_to_old is the ids array handed in, old_to_new its inverse plus id_base -- in one chunk and, with KNNX_ID_ORDER_CHUNK=64, in
    three chunks with a ragged tail."""
    if chunk is None:
        monkeypatch.delenv("KNNX_ID_ORDER_CHUNK", raising=False)
    else:
        monkeypatch.setenv("KNNX_ID_ORDER_CHUNK", chunk)
    ix, ids = _crafted(id_base)
    _check_mapping(ix, ids, id_base)
    ix.close()


@pytest.mark.parametrize("id_base", [0, 1000])
def test_crafted_lists_through_begin_add_assigned_end(id_base):
    """The same sizes through the streaming build, positions handed over in reverse inside each list: expected from (lists, pos)."""
    from clip_retrieval_amd._lib import check
    from clip_retrieval_amd.knn import Mi355xIndex

    n, nlist = int(SIZES.sum()), len(SIZES)
    rng = np.random.default_rng(3)
    lists = np.repeat(np.arange(nlist, dtype=np.int32), SIZES)
    pos = np.concatenate([np.arange(s - 1, -1, -1, dtype=np.int32) for s in SIZES])
    ids = rng.permutation(n).astype(np.int64) + id_base
    shuffle = rng.permutation(n)  # the rows arrive in no particular order
    lists, pos, ids = np.ascontiguousarray(lists[shuffle]), np.ascontiguousarray(pos[shuffle]), np.ascontiguousarray(ids[shuffle])
    rows = _data(n, D, 4)
    cent = _data(nlist, D, 5)
    ix = Mi355xIndex(D, id_base=id_base)
    lib, h = ix._lib, ix._h  # pylint: disable=protected-access
    check(lib, lib.knnx_ivf_begin(h, nlist, cent.ctypes.data, SIZES.ctypes.data), "knnx")
    out = np.full(4, -7, dtype=np.int64)
    assert lib.knnx_ivf_map_ids(h, ids.ctypes.data, 4, out.ctypes.data) == -4 and (out == -7).all()  # KNNX_E_STATE: a build is open
    assert b"knnx_ivf_end" in lib.knnx_last_error()
    for a, b in ((0, 100), (100, n)):
        check(lib, lib.knnx_ivf_add_assigned(h, rows[a:b].ctypes.data, b - a, ids[a:b].ctypes.data, lists[a:b].ctypes.data, pos[a:b].ctypes.data), "knnx")
    assert lib.knnx_ivf_id_order(h, out.ctypes.data, None) == -4
    check(lib, lib.knnx_ivf_end(h), "knnx")
    start = np.r_[0, np.cumsum(SIZES)]
    want = np.empty(n, dtype=np.int64)
    want[start[lists] + pos] = ids
    _check_mapping(ix, want, id_base)
    ix.close()


# ------------------------------------------------------------------------------------------------ IVF-PQ
def _pq_index(variant, n=6000, nlist=48, seed=11, **kw):
    from clip_retrieval_amd.knn import IvfBuilder, build_ivfpq_index, opq_initial_rotation

    d, M = (512, 256) if variant == "m256" else (D, 16)
    x = _data(n, d, seed)
    cent = x[np.random.default_rng(seed + 1).choice(n, nlist, replace=False)]
    b = IvfBuilder(d, nlist)
    b.set_centroids(cent)
    lists = b.assign(x)
    b.close()
    cb = _seed_codebooks(x, cent, lists, M, seed + 2)  # (any codebook is a valid quantiser, behind a rotation too)
    if variant == "rotation":
        kw["rotation"] = opq_initial_rotation(d, seed + 3)
    if variant == "refine":
        kw["refine"] = True
    ix = build_ivfpq_index(x, nlist, M, nprobe=kw.pop("nprobe", 6), centroids=cent, codebooks=cb, **kw)
    return x, ix


def _arena_ids(ix):
    """The ids of an IVF-PQ index in arena order, list by list (knnx_ivfpq_get_codes)."""
    from clip_retrieval_amd._lib import check

    n, M = ix.ntotal, ix.pq_m
    ids, lists, codes = np.empty(n, np.int64), np.empty(n, np.int32), np.empty((n, M), np.uint8)
    check(ix._lib, ix._lib.knnx_ivfpq_get_codes(ix._h, ids.ctypes.data, lists.ctypes.data, codes.ctypes.data), "knnx")  # pylint: disable=protected-access
    return ids


@pytest.mark.parametrize("variant", ["plain", "rotation", "refine", "m256"])
def test_ivfpq_new_to_old_is_the_arena_order(variant):
    _, ix = _pq_index(variant)
    o2n = _check_mapping(ix, _arena_ids(ix), 0)
    probe = np.asarray([0, 5999, 17, 17, -1, 3000], dtype=np.int64)
    assert np.array_equal(ix.map_ids(probe), np_map_ids(o2n, probe))
    ix.close()


@pytest.fixture(scope="module")
def crafted_1000():
    ix, ids = _crafted(1000, seed=9)
    o2n = ix.ivf_old_to_new()
    assert np.array_equal(o2n, np_id_order([ids], 1000)[0])
    yield ix, o2n.copy()
    ix.close()


def _request(n, rng, id_base, ntotal):
    ids = rng.integers(id_base, id_base + ntotal, n).astype(np.int64)
    if n >= 3:
        ids[rng.integers(0, n, max(1, n // 8))] = -1      # -1 sprinkled in
        ids[rng.integers(0, n, max(1, n // 8))] = ids[0]  # duplicates
    return ids


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_map_ids_equals_the_table(crafted_1000, n):
    ix, o2n = crafted_1000
    ids = _request(n, np.random.default_rng(n), 1000, len(o2n))
    before = ids.copy()
    got = ix.map_ids(ids)
    assert got.dtype == np.int64 and got.shape == ids.shape and np.array_equal(ids, before)
    assert np.array_equal(got, np_map_ids(o2n, ids, 1000))


def test_map_ids_shapes_in_place_and_chunked(crafted_1000, monkeypatch):
    ix, o2n = crafted_1000
    rng = np.random.default_rng(1)
    two_d = _request(7 * 40, rng, 1000, len(o2n)).reshape(7, 40)
    assert np.array_equal(ix.map_ids(two_d), np_map_ids(o2n, two_d, 1000)) and ix.map_ids(two_d).shape == (7, 40)
    assert np.array_equal(ix.map_ids([[1000, -1], [1161, 1000]]), np_map_ids(o2n, [[1000, -1], [1161, 1000]], 1000))
    # in place: out aliases ids
    ids = _request(300, rng, 1000, len(o2n))
    want = np_map_ids(o2n, ids, 1000)
    lib, h = ix._lib, ix._h  # pylint: disable=protected-access
    assert lib.knnx_ivf_map_ids(h, ids.ctypes.data, ids.size, ids.ctypes.data) == 0
    assert np.array_equal(ids, want)
    # a call larger than its staging: 1000 ids through chunks of 64 (the last one ragged), in place too
    monkeypatch.setenv("KNNX_ID_ORDER_CHUNK", "64")
    big = _request(1000, rng, 1000, len(o2n))
    want = np_map_ids(o2n, big, 1000)
    assert np.array_equal(ix.map_ids(big), want)
    assert lib.knnx_ivf_map_ids(h, big.ctypes.data, big.size, big.ctypes.data) == 0 and np.array_equal(big, want)
    monkeypatch.delenv("KNNX_ID_ORDER_CHUNK")
    assert np.array_equal(ix.map_ids(_request(500, rng, 1000, len(o2n))).shape, (500,))


def test_refusals(crafted_1000):
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import Mi355xIndex

    ix, o2n = crafted_1000
    lib, h = ix._lib, ix._h  # pylint: disable=protected-access
    for bad, where in ((999, 2), (1000 + len(o2n), 0), (-2, 3), (0, 1)):
        ids = np.asarray([1000, 1001, 1002, 1003], dtype=np.int64)
        ids[where] = bad
        out = np.full(4, -7, dtype=np.int64)
        assert lib.knnx_ivf_map_ids(h, ids.ctypes.data, 4, out.ctypes.data) == -1  # KNNX_E_ARG
        msg = lib.knnx_last_error().decode()
        assert f"id {bad} at position {where}" in msg, msg
        assert (out == -7).all(), "a refused request leaves the output unwritten"
        with pytest.raises(HipLibraryError) as e:
            ix.map_ids(ids)
        assert E_ARG in str(e.value) and str(bad) in str(e.value)
    assert lib.knnx_ivf_id_order(h, None, None) == -1
    flat = Mi355xIndex(D)
    flat.add(_data(64, D, 1))
    for call in (lambda: flat.map_ids([0, 1]), flat.ivf_old_to_new, flat.ivf_new_to_old):
        with pytest.raises(HipLibraryError) as e:
            call()
        assert E_STATE in str(e.value) and "flat index" in str(e.value)
    flat.close()


# ------------------------------------------------------------------------------------------------ search_to_new_ids
@pytest.mark.parametrize("k,threshold", [(10, False), (100, True)])
def test_search_to_new_ids_is_take_of_the_mapping(k, threshold):
    from clip_retrieval_amd.knn import get_old_to_new_mapping, search_to_new_ids

    x, ix = _pq_index("plain", threshold_scan=threshold)
    mapping = get_old_to_new_mapping(ix)
    assert np.array_equal(mapping, np_id_order([_arena_ids(ix)])[0])
    for q in _queries(3, D, 5, x):
        Dp, Ip = ix.search(q[None], k)
        Dn, In = search_to_new_ids(ix, q[None], k)
        assert (Ip[0] >= 0).sum() >= min(k, 64)
        assert Dn.shape == (1, k) and In.shape == (k,)
        assert np.array_equal(Dn.view(np.uint32), Dp.view(np.uint32))  # the search is the plain search, bit for bit
        assert np.array_equal(In, np.where(Ip[0] == -1, -1, np.take(mapping, np.maximum(Ip[0], 0))))
    ix.close()


def test_map_ids_while_other_threads_search():
    """Eight threads translate while eight threads search the same index: every answer equals the serial one."""
    x, ix = _pq_index("plain")
    o2n = ix.ivf_old_to_new()
    q = _queries(8, D, 6, x)
    serial = [ix.search(q[t:t + 1], 40) for t in range(8)]
    reqs = [_request(40 + t, np.random.default_rng(100 + t), 0, len(o2n)) for t in range(8)]
    errors = []

    def mapper(t):
        try:
            for _ in range(50):
                if not np.array_equal(ix.map_ids(reqs[t]), np_map_ids(o2n, reqs[t])):
                    errors.append(("map", t))
        except Exception as e:  # pylint: disable=broad-except
            errors.append(("map", t, repr(e)))

    def searcher(t):
        try:
            for _ in range(20):
                Dt, It = ix.search(q[t:t + 1], 40)
                if not (np.array_equal(It, serial[t][1]) and np.allclose(Dt, serial[t][0], atol=1e-5)):
                    errors.append(("search", t))
        except Exception as e:  # pylint: disable=broad-except
            errors.append(("search", t, repr(e)))

    threads = [threading.Thread(target=f, args=(t,)) for t in range(8) for f in (mapper, searcher)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[:5]
    ix.close()


# ------------------------------------------------------------------------------------------------ shards
def test_two_shards_on_one_gpu():
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import IvfBuilder, Mi355xIndex, ShardedMi355xIndex, build_ivfpq_index

    n, nlist, M = 6000, 48, 16
    x = _data(n, D, 21)
    cent = x[np.random.default_rng(2).choice(n, nlist, replace=False)]
    b = IvfBuilder(D, nlist)
    b.set_centroids(cent)
    lists = b.assign(x)
    b.close()
    cb = _seed_codebooks(x, cent, lists, M, 3)
    cut = [0, 2500, n]
    shards = [build_ivfpq_index(x[cut[g]:cut[g + 1]], nlist, M, nprobe=6, id_base=cut[g], centroids=cent, codebooks=cb) for g in range(2)]
    o2n = np.concatenate([s.ivf_old_to_new() for s in shards])
    n2o = np.concatenate([s.ivf_new_to_old() for s in shards])
    for g in range(2):  # list-sorted inside each shard's own range
        assert np.array_equal(np.sort(o2n[cut[g]:cut[g + 1]]), np.arange(cut[g], cut[g + 1]))
    ix = ShardedMi355xIndex.from_shards(shards, cut[:2])
    assert np.array_equal(ix.ivf_old_to_new(), o2n) and np.array_equal(ix.ivf_new_to_old(), n2o)
    assert np.array_equal(np.sort(o2n), np.arange(n)) and np.array_equal(o2n[n2o], np.arange(n))
    ids = np.asarray([[2499, 2500, 0, 5999, -1, 2500], [2498, 2501, 2499, -1, 1, 5998]], dtype=np.int64)  # across the boundary
    assert np.array_equal(ix.map_ids(ids), np_map_ids(o2n, ids))
    big = _request(1000, np.random.default_rng(8), 0, n)
    assert np.array_equal(ix.map_ids(big), np_map_ids(o2n, big))
    assert ix.map_ids(np.zeros(0, np.int64)).shape == (0,)
    out = np.full(3, -7, dtype=np.int64)
    past = np.asarray([5999, n, 0], dtype=np.int64)
    assert ix._lib.knnx_shards_map_ids(ix._h, past.ctypes.data, 3, out.ctypes.data) == -1 and (out == -7).all()  # pylint: disable=protected-access
    with pytest.raises(HipLibraryError) as e:
        ix.map_ids(past)
    assert E_ARG in str(e.value) and f"id {n} at position 1" in str(e.value)
    ix.close()
    flat = [Mi355xIndex(D, id_base=0), Mi355xIndex(D, id_base=64)]
    for f in flat:
        f.add(_data(64, D, 1))
    sh = ShardedMi355xIndex.from_shards(flat, [0, 64])
    for call in (lambda: sh.map_ids([0, 70]), sh.ivf_old_to_new):
        with pytest.raises(HipLibraryError) as e:
            call()
        assert E_STATE in str(e.value)
    sh.close()


# ------------------------------------------------------------------------------------------------ the request path, end to end
def test_knn_hot_path_with_a_reordered_arrow_folder(tmp_path):
    """Image and text index with DIFFERENT centroids (so different lists), metadata ordered by the image index's lists,
    ivf_old_to_new_mapping=None: the records fetched from the re-ordered folder by the returned ids are those fetched from the original
    folder by a run with metadata_is_ordered_by_ivf=False -- for both modalities, with and without deduplicate."""
    pytest.importorskip("pyarrow")
    from clip_retrieval_amd.knn import build_ivf_index
    from clip_retrieval_amd.service import ArrowMetadataProvider, KnnHotPath, reorder_arrow_metadata

    n, nlist = 3000, 24
    rng = np.random.default_rng(12)
    img = _data(n, D, 31).astype(np.float32)
    img[100:110] = img[7] + 0.01 * rng.standard_normal((10, D)).astype(np.float32)  # near-duplicates of row 7: the dedup has work
    img = (img / np.linalg.norm(img, axis=1, keepdims=True)).astype(np.float16)
    txt = _data(n, D, 32)
    image_index = build_ivf_index(img, nlist, nprobe=6, centroids=img[rng.choice(n, nlist, replace=False)])
    text_index = build_ivf_index(txt, nlist, nprobe=6, centroids=txt[rng.choice(n, nlist, replace=False)])
    assert not np.array_equal(image_index.ivf_old_to_new(), text_index.ivf_old_to_new())
    src, dst = str(tmp_path / "meta"), str(tmp_path / "meta_by_list")
    write_arrow_folder(src, n, 3)
    reorder_arrow_metadata(image_index, src, dst, rows_per_file=1024)
    old, new = ArrowMetadataProvider(src), ArrowMetadataProvider(dst)
    hp = KnnHotPath()
    res = SimpleNamespace(image_index=image_index, text_index=text_index, metadata_is_ordered_by_ivf=False, ivf_old_to_new_mapping=None,
                          safety_model=None, violence_detector=None)
    dropped = 0
    for modality, rows in (("image", img), ("text", txt)):
        for q in (rows[7:8], rows[1500:1501], rows[2999:3000]):
            q = q.astype(np.float32)
            for dedup in (False, True):
                res.metadata_is_ordered_by_ivf = False
                d0, i0 = hp.knn_search(q, modality, 40, res, dedup, False, False)
                res.metadata_is_ordered_by_ivf = True
                d1, i1 = hp.knn_search(q, modality, 40, res, dedup, False, False)
                assert len(i0) > 0 and np.array_equal(np.asarray(d0), np.asarray(d1))
                assert [int(v) for v in i1] == [int(v) for v in image_index.map_ids(np.asarray(i0, dtype=np.int64))]
                assert new.get(i1) == old.get(i0), (modality, dedup)
                meta = KnnHotPath.map_to_metadata(i1, d1, 40, new, ["url", "row"])
                assert [m["row"] for m in meta] == [int(v) for v in i0]
                dropped += dedup and len(i0) < 40
    assert dropped > 0, "no request exercised the dedup"
    image_index.close()
    text_index.close()


def test_save_load_gives_the_same_mapping(tmp_path):
    """Nothing new is stored: the mapping follows from the layout, and the loaded index lays its lists out as the built one did."""
    from clip_retrieval_amd import knn

    _, ix = _pq_index("plain")
    o2n, n2o = ix.ivf_old_to_new(), ix.ivf_new_to_old()
    out = str(tmp_path / "idx")
    knn.save_index(ix, out)
    ix.close()
    assert sorted(os.listdir(out)) == sorted(["ivf_pq_centroids.npy", "ivf_pq_codebooks.npy", "ivf_pq_codes.npy", "ivf_pq_lists.npy",
                                              knn.IVFPQ_MANIFEST])
    loaded = knn.load_index(out)
    assert np.array_equal(loaded.ivf_old_to_new(), o2n) and np.array_equal(loaded.ivf_new_to_old(), n2o)
    ids = _request(200, np.random.default_rng(2), 0, len(o2n))
    assert np.array_equal(loaded.map_ids(ids), np_map_ids(o2n, ids))
    loaded.close()
