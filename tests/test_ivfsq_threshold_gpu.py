"""The threshold scan of IVF-SQ8 on the GPU (Mi355xIndex.sq_threshold_scan; include/knnx.h: knnx_ivfsq_set_threshold_scan): range_search
and k > 64 against the float64 restatement of test_ivfsq_cpu.py on the index's own codes -- at the tile edges of the crafted index of
test_ivfsq_gpu.py (list sizes 0, 1, 31, 32, 33, 700 ..., a vdiff == 0 column, rows outside the trained ranges), on a 9 000-row index for
the long hit lists and the pool regrowth, over two shards, through save / load, through KnnHotPath.knn_search and next to the coalescer
-- and the rules of the switch itself.

The crafted indexes are shared with test_ivfsq_gpu.py, whose tests expect the switch OFF: every test here that switches one on puts it
back (the fixture `on`)."""
import ctypes as C
import json
import os
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from test_ivfsq_cpu import NEG, corpus, np_ranges, np_sq_decode, np_sq_encode, np_sq_scores, np_sq_search
from test_ivfsq_gpu import N, NLIST, SIZES, _check, _crafted, _index, _queries

pytestmark = pytest.mark.gpu

KNNX_E_STATE = -4
TOL = 1e-5  # |fp32 score - float64 score| of the project's scans (include/knnx.h, "IVF-SQ8": score)
NEAR_MAX = 0.005  # reference hits within TOL of the threshold may fall on either side: at most this share of a case's reference hits


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture
def on():
    """on(d) -> the crafted index of width d with the switch on; every index handed out is switched off again afterwards."""
    used = []

    def get(d):
        c = _index(d)
        c.ix.sq_threshold_scan = True
        used.append(c)
        return c

    yield get
    for c in used:
        c.ix.sq_threshold_scan = False
        c.ix.nprobe = 5


_REF = {}


def _reference(d, nprobe, B, seed):
    """(q, D, I, amb) of np_sq_search with k = N + 10 -- every row of the probed lists, ranked -- computed once per (d, nprobe, B, seed)."""
    key = (d, nprobe, B, seed)
    if key not in _REF:
        c = _index(d)
        q = _queries(B, d, seed=seed, x=c.x)
        _REF[key] = (q,) + np_sq_search(q, c.cent, c.codes, c.lists, *c.ranges, 0, nprobe, N + 10)
    return _REF[key]


def _check_range(lims, D, I, Do, Io, amb, thr, ctx):
    """lims consistent, ids ascending per query, every score within TOL of its float64 value, the hit sets equal -- a reference row
    within TOL of the threshold may fall on either side (at most NEAR_MAX of the reference hits: asserted first)."""
    nq = Do.shape[0]
    hit = (Io >= 0) & (Do > thr)
    near = (Io >= 0) & (np.abs(Do - thr) <= TOL)
    share = near[~amb].sum() / max(1, hit[~amb].sum())
    print(f"{ctx}: {int(hit[~amb].sum())} reference hits, {int(near[~amb].sum())} within {TOL} of the threshold ({100 * share:.3f} %)")
    assert near[~amb].sum() <= NEAR_MAX * hit[~amb].sum(), ctx
    assert lims.shape == (nq + 1,) and lims[0] == 0 and (np.diff(lims) >= 0).all() and lims[-1] == len(D) == len(I), ctx
    worst = 0.0
    for i in range(nq):
        if amb[i]:
            continue
        ids, sc = I[lims[i]:lims[i + 1]], D[lims[i]:lims[i + 1]]
        assert (np.diff(ids) > 0).all(), f"{ctx}: query {i} ids not ascending"
        score = np.full(N, np.nan)
        score[Io[i][Io[i] >= 0]] = Do[i][Io[i] >= 0]
        assert not np.isnan(score[ids]).any(), f"{ctx}: query {i} returned a row outside its probed lists"
        worst = max(worst, np.abs(sc.astype(np.float64) - score[ids]).max(initial=0))
        sure, maybe = set(Io[i][hit[i] & ~near[i]].tolist()), set(Io[i][near[i]].tolist())
        got = set(ids.tolist())
        assert sure <= got and got <= (sure | maybe), f"{ctx}: query {i}: missing {sorted(sure - got)[:5]}, extra {sorted(got - sure - maybe)[:5]}"
    print(f"{ctx}: {int(lims[-1])} hits, max score error {worst:.3e}")
    assert worst <= TOL, ctx


# ------------------------------------------------------------------------------------------------ 1. range parity
# (d, thresh, nprobe, B): every d {256, 768, 1024}, thresh {-1, 0, 0.05, 0.3}, nprobe {1, 5, 24}, B {1, 33, 300} appears
RANGE_CASES = [(256, -1.0, 1, 1), (256, 0.0, 5, 33), (256, 0.05, 24, 300), (256, 0.3, 5, 1),
               (768, 0.0, 24, 1), (768, 0.05, 1, 33), (768, 0.3, 5, 300), (768, -1.0, 24, 33),
               (1024, 0.05, 5, 1), (1024, 0.3, 24, 33), (1024, -1.0, 1, 300), (1024, 0.0, 5, 300)]


@pytest.mark.parametrize("d,thr,nprobe,B", RANGE_CASES)
def test_range_parity(on, d, thr, nprobe, B):
    c = on(d)
    c.ix.nprobe = nprobe
    q, Do, Io, amb = _reference(d, nprobe, B, seed=B + 7)
    assert amb.mean() < 0.5
    lib, h = c.ix._lib, c.ix._h  # pylint: disable=protected-access
    qc = np.ascontiguousarray(q)
    lims = np.full(B + 1, -7, dtype=np.int64)
    assert lib.knnx_range_search(h, qc.ctypes.data, B, C.c_float(thr), lims.ctypes.data, None, None) == 0, lib.knnx_last_error()
    D = np.empty(int(lims[-1]), np.float32)
    I = np.empty(int(lims[-1]), np.int64)
    assert lib.knnx_range_search(h, qc.ctypes.data, B, C.c_float(thr), lims.ctypes.data, D.ctypes.data, I.ctypes.data) == 0, lib.knnx_last_error()
    _check_range(lims, D, I, Do, Io, amb, thr, f"d={d} thr={thr} nprobe={nprobe} B={B}")


# ------------------------------------------------------------------------------------------------ 2. protocol
def test_range_protocol(on):
    """The two-call form, knnx_range_search_once with a capacity too small / large enough, lims of another threshold."""
    d, thr = 768, 0.05
    c = on(d)
    c.ix.nprobe = 5
    lib, h = c.ix._lib, c.ix._h  # pylint: disable=protected-access
    q, Do, Io, amb = _reference(d, 5, 5, seed=3)
    q = np.ascontiguousarray(q)
    lims = np.full(6, -7, dtype=np.int64)
    assert lib.knnx_range_search(h, q.ctypes.data, 5, C.c_float(thr), lims.ctypes.data, None, None) == 0
    total = int(lims[5])
    assert lims[0] == 0 and (np.diff(lims) >= 0).all() and total > 10
    D = np.empty(total, np.float32)
    I = np.empty(total, np.int64)
    assert lib.knnx_range_search(h, q.ctypes.data, 5, C.c_float(thr), lims.ctypes.data, D.ctypes.data, I.ctypes.data) == 0
    _check_range(lims, D, I, Do, Io, amb, thr, "two calls")
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
    # the Python wrapper gives the same
    l2, D2, I2 = c.ix.range_search(q, thr)
    assert np.array_equal(l2, lims1) and np.array_equal(I2, I1) and np.array_equal(_bits(D2), _bits(D1))


# ------------------------------------------------------------------------------------------------ 3. long lists, pool regrowth
BIG_N, BIG_D, BIG_NLIST = 9000, 256, 8
_big = {}


def _big_index():
    """9 000 x 256, nlist 8, nprobe 8 (every row is probed), built with the switch on: lists of ~1 000 rows."""
    from clip_retrieval_amd.knn import build_ivfsq_index, train_ivf_centroids

    if not _big:
        x = corpus("mixture", BIG_D, BIG_N)
        cent = train_ivf_centroids(x, BIG_NLIST, niter=2, seed=0)
        ranges = np_ranges(x)
        ix = build_ivfsq_index(x, BIG_NLIST, nprobe=BIG_NLIST, centroids=cent, ranges=ranges, threshold_scan=True)
        assert ix.sq_threshold_scan is True
        _big.update(x=x, ix=ix, ranges=ranges, codes=np_sq_encode(x, *ranges))
    return SimpleNamespace(**_big)


@pytest.fixture(scope="module", autouse=True)
def _close_big():
    yield
    if _big:
        _big["ix"].close()
        _big.clear()


def test_long_hit_list_takes_the_radix_sort():
    """9 000 hits of one query: more than RANGE_SORT_SMALL = 4 096."""
    b = _big_index()
    q = _queries(1, BIG_D, seed=11, x=b.x)
    lims, D, I = b.ix.range_search(q, -1.0)
    assert lims.tolist() == [0, BIG_N] and np.array_equal(I, np.arange(BIG_N))
    assert np.abs(D.astype(np.float64) - np_sq_scores(q, b.codes, *b.ranges)[0]).max() <= TOL


def test_pool_regrows_and_rescans():
    """256 x 9 000 hits: more than the initial 2^21-entry pool.  Every row exactly once per query."""
    b = _big_index()
    B = 256
    q = _queries(B, BIG_D, seed=12, x=b.x)
    lims, D, I = b.ix.range_search(q, -1.0)
    assert np.array_equal(lims, np.arange(B + 1, dtype=np.int64) * BIG_N)
    assert np.array_equal(I.reshape(B, BIG_N), np.broadcast_to(np.arange(BIG_N), (B, BIG_N)))
    assert np.abs(D.reshape(B, BIG_N).astype(np.float64) - np_sq_scores(q, b.codes, *b.ranges)).max() <= TOL
    # a small request afterwards is served from the grown pool
    l2, _, I2 = b.ix.range_search(q[:2], 0.5)
    S = np_sq_scores(q[:2], b.codes, *b.ranges)
    for i in range(2):
        assert np.isin(np.flatnonzero(S[i] > 0.5 + TOL), I2[l2[i]:l2[i + 1]]).all()
        assert np.isin(I2[l2[i]:l2[i + 1]], np.flatnonzero(S[i] > 0.5 - TOL)).all()


# ------------------------------------------------------------------------------------------------ 4. large k parity
# (d, k, B, nprobe): every d, k {65, 100, 700, N + 10}, B {1, 3, 33, 300}, nprobe {1, 5, 24} appears
LARGE_CASES = [(256, 65, 1, 1), (256, 100, 33, 24), (256, 700, 3, 5), (256, N + 10, 300, 5),
               (768, 100, 300, 24), (768, 700, 1, 1), (768, N + 10, 33, 5), (768, 65, 3, 24),
               (1024, 700, 33, 5), (1024, N + 10, 1, 24), (1024, 65, 300, 1), (1024, 100, 3, 24)]


@pytest.mark.parametrize("d,k,B,nprobe", LARGE_CASES)
def test_large_k_parity(on, d, k, B, nprobe):
    c = on(d)
    c.ix.nprobe = nprobe
    q, Dall, Iall, amb = _reference(d, nprobe, B, seed=B + 21)
    assert amb.mean() < 0.5
    before = c.ix.sq_threshold_stats()
    D, I = c.ix.search(q, k)
    after = c.ix.sq_threshold_stats()
    _check(D, I, Dall[:, :k], Iall[:, :k], amb, f"d={d} k={k} B={B} nprobe={nprobe}")
    queries, launches, qscans, hits = (a - b for a, b in zip(after, before))
    print(f"d={d} k={k} B={B} nprobe={nprobe}: {launches} launches, {qscans / B:.2f} threshold scans and {hits / B:.0f} hits per query")
    assert queries == B and launches >= 1 and qscans >= B
    if nprobe == NLIST and k == 100:  # T_q = 2 294 > 2 k: the descent runs, not one take-everything scan
        assert qscans > queries


# ------------------------------------------------------------------------------------------------ 5. bitwise
@pytest.mark.parametrize("d", [256, 768, 1024])
def test_large_k_bitwise(on, d):
    """In one batch of 33 the first 64 of a k = 100 search are the k = 64 search, D bits and ids; a query alone, in 33 and in 300 gets
    the same ids with D within 2e-6 (the bar of test_ivfsq_gpu.test_batch_independence)."""
    c = on(d)
    c.ix.nprobe = 5
    q = _queries(300, d, 9, c.x)
    D64, I64 = c.ix.search(q[:33], 64)
    D100, I100 = c.ix.search(q[:33], 100)
    assert np.array_equal(I100[:, :64], I64) and np.array_equal(_bits(D100[:, :64]), _bits(D64))
    D300, I300 = c.ix.search(q, 100)
    assert np.array_equal(I300[:33], I100) and np.abs(D300[:33] - D100).max() <= 2e-6
    for i in (0, 17, 32):
        D1, I1 = c.ix.search(q[i:i + 1], 100)
        assert np.array_equal(I1[0], I100[i]) and np.abs(D1[0] - D100[i]).max() <= 2e-6, i


# ------------------------------------------------------------------------------------------------ 6. exact ties
def test_exact_ties():
    """200 rows with identical codes spread over three lists: k = 100 returns the 100 smallest ids among them in ascending order,
    range_search all 200."""
    from clip_retrieval_amd import knn

    d, n, nlist = 256, 1200, 6
    x = corpus("isotropic", d, n).copy()
    rng = np.random.default_rng(5)
    tied = np.sort(rng.choice(n, 200, replace=False))
    x[tied] = x[tied[0]]
    lists = (np.arange(n) % nlist).astype(np.int32)
    lists[tied] = np.array([0, 2, 5], dtype=np.int32)[np.arange(200) % 3]
    cent = np.stack([x[lists == l].astype(np.float32).mean(0) for l in range(nlist)])
    cent = (cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(np.float16)
    ranges = np_ranges(x)
    codes = np_sq_encode(x, *ranges)
    assert (codes[tied] == codes[tied[0]]).all()
    ix = knn._ivfsq_encode_chunks(iter([(0, x)]), n, d, nlist, cent, ranges, lists, nlist, 0, 0, threshold_scan=True)  # pylint: disable=protected-access
    q = x[tied[:1]].astype(np.float32)
    q /= np.linalg.norm(q)
    S = np_sq_scores(q, codes, *ranges)[0]
    assert S[tied].min() > 0.9 and np.delete(S, tied).max() < 0.5
    D, I = ix.search(q, 100)
    assert np.array_equal(I[0], tied[:100]) and (_bits(D[0]) == _bits(D[0])[0]).all() and abs(float(D[0, 0]) - S[tied[0]]) <= TOL
    lims, Dr, Ir = ix.range_search(q, 0.5)
    assert lims.tolist() == [0, 200] and np.array_equal(Ir, tied) and (_bits(Dr) == _bits(D[0])[0]).all()
    ix.close()


# ------------------------------------------------------------------------------------------------ 7. short lists
def test_short_and_empty_lists(on):
    """Probed lists holding fewer than k rows -> -1 / -FLT_MAX padding; nprobe 1 landing on an empty list -> all -1 and empty ranges."""
    c = on(768)
    c.ix.nprobe = 1
    pick = [int(np.flatnonzero(SIZES == s)[0]) for s in (0, 1, 31, 33)]
    q = np.ascontiguousarray(c.cent[pick].astype(np.float32))
    Do, Io, amb = np_sq_search(q, c.cent, c.codes, c.lists, *c.ranges, 0, 1, 100)
    assert not amb.any() and [(r >= 0).sum() for r in Io] == [0, 1, 31, 33]
    D, I = c.ix.search(q, 100)
    assert (I[0] == -1).all() and (D[0] == NEG).all()
    _check(D, I, Do, Io, amb, "short lists k=100")
    lims, Dr, Ir = c.ix.range_search(q, -1.0)
    assert np.diff(lims).tolist() == [0, 1, 31, 33]
    for i in range(1, 4):
        assert np.array_equal(Ir[lims[i]:lims[i + 1]], np.sort(Io[i][Io[i] >= 0]))
    lims, _, _ = c.ix.range_search(q[:1], -1.0)  # the empty list alone
    assert lims.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 8. the switch
def test_switch_semantics():
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import Mi355xIndex, build_ivf_index, build_ivfpq_index, build_ivfsq_index

    x, lists, cent, ranges = _crafted(256)
    ix = build_ivfsq_index(x, NLIST, nprobe=5, centroids=cent, ranges=ranges)
    q = _queries(2, 256, 1, x)

    def refused():
        with pytest.raises(HipLibraryError, match=r"code -5\): k > 64 is not supported on an IVF-SQ8 index$"):
            ix.search(q, 65)
        with pytest.raises(HipLibraryError, match=r"code -5\): range_search is not supported on an IVF-SQ8 index$"):
            ix.range_search(q, 0.5)

    assert ix.sq_threshold_scan is False
    refused()  # a default-built index answers as it always has
    D40, I40 = ix.search(q, 40)

    def flat_answer():
        f = build_ivf_index(x, NLIST, nprobe=5, centroids=cent)
        out = f.search(q, 100)
        f.close()
        return out

    flat_before = flat_answer()
    ix.sq_threshold_scan = True
    assert ix.sq_threshold_scan is True
    D, I = ix.search(q, 65)
    assert np.array_equal(I[:, :40], I40) and np.array_equal(_bits(D[:, :40]), _bits(D40))
    lims, _, _ = ix.range_search(q, 0.0)
    assert lims[-1] > 0
    ix.sq_threshold_scan = False
    assert ix.sq_threshold_scan is False
    refused()
    D40b, I40b = ix.search(q, 40)
    assert np.array_equal(I40b, I40) and np.array_equal(_bits(D40b), _bits(D40))
    ix.sq_threshold_scan = True  # ... and on again
    assert np.array_equal(ix.search(q, 65)[1], I)
    ix.close()
    flat_after = flat_answer()  # an IVF-Flat index built before and after: identical k = 100 answers
    assert np.array_equal(flat_before[1], flat_after[1]) and np.array_equal(_bits(flat_before[0]), _bits(flat_after[0]))
    # built switched on
    built_on = build_ivfsq_index(x, NLIST, nprobe=5, centroids=cent, ranges=ranges, threshold_scan=True)
    assert built_on.sq_threshold_scan is True
    assert np.array_equal(built_on.search(q, 65)[1], I)
    built_on.close()
    # not an IVF-SQ8 index: the getter says False, the setter is an error that names the index kind it wants
    flat = Mi355xIndex(256)
    flat.add(x)
    ivf = build_ivf_index(x, NLIST, nprobe=5, centroids=cent)
    rng = np.random.default_rng(0)
    pq = build_ivfpq_index(x, NLIST, 16, nprobe=5, centroids=cent, codebooks=(0.05 * rng.standard_normal((16, 256, 16))).astype(np.float32))
    for other in (flat, ivf, pq):
        assert other.sq_threshold_scan is False
        with pytest.raises(HipLibraryError, match=r"code -4\).*IVF-SQ8"):
            other.sq_threshold_scan = True
        assert other.sq_threshold_scan is False
        with pytest.raises(HipLibraryError, match=r"code -4\).*IVF-SQ8"):
            other.sq_threshold_stats()
        other.close()


# ------------------------------------------------------------------------------------------------ 9. shards
def test_two_shards_on_one_gpu(on):
    from clip_retrieval_amd import HipLibraryError, knn

    d = 768
    c = on(d)
    c.ix.nprobe = 5
    cut = [0, 1300, N]
    shards = [knn._ivfsq_encode_chunks(iter([(0, c.x[cut[g]:cut[g + 1]])]), cut[g + 1] - cut[g], d, NLIST, c.cent, c.ranges,  # pylint: disable=protected-access
                                       c.lists[cut[g]:cut[g + 1]], 5, 0, cut[g]) for g in range(2)]
    sh = knn.ShardedMi355xIndex.from_shards(shards, cut[:2])
    sh.nprobe = 5
    q = _queries(7, d, 6, c.x)
    assert sh.sq_threshold_scan is False
    with pytest.raises(HipLibraryError, match="k > 64 is not supported on an IVF-SQ8 index"):
        sh.search(q, 100)
    sh.sq_threshold_scan = True  # sets every shard
    lib, h = sh._lib, sh._h  # pylint: disable=protected-access
    assert sh.sq_threshold_scan is True and sh.nshards == 2
    assert all(lib.knnx_ivfsq_threshold_scan(C.c_void_p(lib.knnx_shards_get(h, g))) == 1 for g in range(2))
    D, I = sh.search(q, 100)
    D1, I1 = c.ix.search(q, 100)
    assert np.array_equal(I, I1) and np.abs(D - D1).max() <= 2e-6
    lims, Dr, Ir = sh.range_search(q, 0.05)
    l1, Dr1, Ir1 = c.ix.range_search(q, 0.05)
    assert np.array_equal(lims, l1) and np.array_equal(Ir, Ir1) and np.abs(Dr - Dr1).max() <= 2e-6
    # one shard switched off: that shard's refusal
    assert lib.knnx_ivfsq_set_threshold_scan(C.c_void_p(lib.knnx_shards_get(h, 1)), 0) == 0
    with pytest.raises(HipLibraryError, match="k > 64 is not supported on an IVF-SQ8 index"):
        sh.search(q, 100)
    with pytest.raises(HipLibraryError, match="range_search is not supported on an IVF-SQ8 index"):
        sh.range_search(q, 0.05)
    sh.close()


# ------------------------------------------------------------------------------------------------ 10. save / load
def test_save_load_keeps_the_switch(on, tmp_path):
    from clip_retrieval_amd import HipLibraryError, knn

    d = 256
    c = on(d)
    c.ix.nprobe = 5
    q = _queries(3, d, 8, c.x)
    D0, I0 = c.ix.search(q, 100)
    out = str(tmp_path / "on")
    man = knn.save_index(c.ix, out)
    assert man["threshold_scan"] is True
    with open(os.path.join(out, knn.IVFSQ_MANIFEST), encoding="utf-8") as f:
        assert json.load(f)["threshold_scan"] is True
    loaded = knn.load_index(out)
    assert loaded.sq_threshold_scan is True
    D1, I1 = loaded.search(q, 100)
    assert np.array_equal(I0, I1) and np.array_equal(_bits(D0), _bits(D1))
    loaded.close()
    sharded = knn.load_index(out, devices=[0, 0])
    assert sharded.sq_threshold_scan is True
    assert np.array_equal(sharded.search(q, 100)[1], I0)
    sharded.close()
    # a bad value
    with open(os.path.join(out, knn.IVFSQ_MANIFEST), encoding="utf-8") as f:
        m = json.load(f)
    with open(os.path.join(out, knn.IVFSQ_MANIFEST), "w", encoding="utf-8") as f:
        json.dump({**m, "threshold_scan": "yes"}, f)
    with pytest.raises(ValueError, match="threshold_scan"):
        knn.load_index(out)
    # a manifest without the key loads with the switch off ...
    del m["threshold_scan"]
    with open(os.path.join(out, knn.IVFSQ_MANIFEST), "w", encoding="utf-8") as f:
        json.dump(m, f)
    off = knn.load_index(out)
    assert off.sq_threshold_scan is False
    with pytest.raises(HipLibraryError, match="k > 64 is not supported on an IVF-SQ8 index"):
        off.search(q, 100)
    # ... and an index saved with the switch off writes no key
    assert "threshold_scan" not in knn.save_index(off, str(tmp_path / "off"))
    with open(os.path.join(str(tmp_path / "off"), knn.IVFSQ_MANIFEST), encoding="utf-8") as f:
        assert "threshold_scan" not in json.load(f)
    off.close()


# ------------------------------------------------------------------------------------------------ 11. the service
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


def test_service_serves_the_reference_request_sizes(on):
    """KnnHotPath.knn_search with num_result_ids = 100 and 3 000 (deduplicate=True) and the >= 100 000 request of the probe-widening
    branch.  The ids are compared as the restatement ranks them, except that neighbours whose float64 scores lie within 1e-5 of each
    other may swap (the tolerance of _check)."""
    from clip_retrieval_amd.service import KnnHotPath

    d, nprobe = 768, 5
    c = on(d)
    c.ix.nprobe = nprobe
    res = SimpleNamespace(image_index=c.ix, text_index=c.ix, metadata_is_ordered_by_ivf=False, safety_model=None, violence_detector=None)
    hp = KnnHotPath()
    q, Do, Io, amb = _reference(d, nprobe, 1, seed=14)
    assert not amb[0]
    ids, S = Io[0][Io[0] >= 0], Do[0][Io[0] >= 0]  # ranked: score descending, id ascending
    dec = np_sq_decode(c.codes, *c.ranges)
    where = {int(a): j for j, a in enumerate(ids)}
    for k in (100, 3000):
        dist, ind = hp.knn_search(q, "image", k, res, True, False, False)
        top = ids[:k]
        want = top[_np_dedup_keep(dec[top])]
        got = np.asarray(ind, dtype=np.int64)
        assert len(got) == len(want) and set(got.tolist()) == set(want.tolist()), f"k={k}"
        sg = np.array([S[where[int(a)]] for a in got])
        assert (np.diff(sg) <= TOL).all() and np.abs(np.asarray(dist, dtype=np.float64) - sg).max() <= TOL, f"k={k}"
        swapped = np.flatnonzero(got != want)
        assert all(abs(S[where[int(got[j])]] - S[where[int(want[j])]]) <= TOL for j in swapped), f"k={k}"
    # >= 100 000: nprobe widened to min(nlist, ceil(1e5 / 3000)) = all 24 lists for the request and put back: every row, once
    dist, ind = hp.knn_search(q, "image", 100000, res, False, False, False)
    assert c.ix.nprobe == nprobe
    assert sorted(int(i) for i in ind) == list(range(N)) and (np.diff(np.asarray(dist)) <= 0).all()
    full = np_sq_scores(q, c.codes, *c.ranges)[0]
    assert np.abs(np.asarray(dist, dtype=np.float64) - full[np.asarray(ind, dtype=np.int64)]).max() <= TOL


# ------------------------------------------------------------------------------------------------ 12. next to the coalescer
def test_large_k_next_to_coalesced_queries(on):
    """One thread repeats a k = 100 search while 16 threads send coalesced k = 40 queries: every answer equals its solo answer."""
    d = 256
    c = on(d)
    c.ix.nprobe = 5
    q = _queries(17, d, 13, c.x)
    solo40 = [c.ix.search(q[i:i + 1], 40) for i in range(16)]
    solo100 = c.ix.search(q[16:17], 100)
    big, small, errs = [], [None] * 16, []

    def large():
        try:
            for _ in range(4):
                big.append(c.ix.search(q[16:17], 100))
        except Exception as e:  # pylint: disable=broad-except
            errs.append(e)

    def one(i):
        try:
            small[i] = [c.ix.search(q[i:i + 1], 40) for _ in range(3)]
        except Exception as e:  # pylint: disable=broad-except
            errs.append(e)

    th = [threading.Thread(target=large)] + [threading.Thread(target=one, args=(i,)) for i in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert len(big) == 4
    for D, I in big:
        assert np.array_equal(I, solo100[1]) and np.abs(D - solo100[0]).max() <= 2e-6
    for i in range(16):
        for D, I in small[i]:
            assert np.array_equal(I, solo40[i][1]) and np.abs(D - solo40[i][0]).max() <= 2e-6
