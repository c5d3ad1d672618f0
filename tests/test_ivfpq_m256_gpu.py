"""IVF-PQ with M = 256 (PQ256x8: the two-half ADC scan, include/knnx.h) on the GPU against the numpy restatement of test_ivfpq_gpu.py
built from the index's own centroids, codebooks and codes: encoding, search parity on built indexes and on crafted lists (empty lists,
sizes around 64 / 256 / 512, a 1 000-row list), exact ties, sub-groups of the partial-sum buffer, the entry points, the threshold scan,
the refine store, the rotation, the round trips, training quality and the refusals.  Every index is built from given centroids and
codebooks (no training, except the quality test) and shared by the tests of the module."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle.knn_oracle import synth_mixture_rows, topk_sets_equal
from test_ivfpq_gpu import _check, _data, _queries, _small_index, codes_match, np_adc_search, np_encode
from test_ivfpq_refine_cpu import TOL as REFINE_TOL
from test_ivfpq_refine_cpu import check_refine, np_refine_parts, np_refine_search
from test_ivfpq_threshold_cpu import check_range, np_adc_parts
from test_opq_cpu import np_pq_encode

pytestmark = pytest.mark.gpu

M = 256
KNNX_E_ARG = -1
_built = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _encode_in_chunks(res, cb, step=100):
    """np_encode without its n x M x 256 x ds float64 array at once (1.3 GB at n = 600, d = 1024)."""
    out = [np_encode(res[o:o + step], cb) for o in range(0, len(res), step)]
    return np.concatenate([c for c, _ in out]), np.concatenate([dd for _, dd in out])


def _index(d):
    """(x, cent, cb, index, codes, lists) of the built index of dimension d: n = 5 000, nlist = 96, seed d + 256; built once, nprobe set
    by every test that uses it."""
    key = ("built", d)
    if key not in _built:
        x, cent, cb, ix = _small_index(5000, d, 96, M, 8, seed=d + M)
        codes, lists = ix.pq_codes()
        _built[key] = (x, cent, cb, ix, codes, lists)
    return _built[key]


# the crafted lists: empty lists, one row, every size around a wave (64), a step of the workgroup (256) and two steps (512), a long list
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 0, 31, 32, 33, 129]
CD = 768


def _crafted_parts(sizes, seed, ties):
    """Random u8 codes, random codebooks, random unit fp16 centroids; ids interleave the lists.  ties: one code row copied over 100 rows
    of the 1 000-row list and over 30 rows of the 257-row list."""
    rng = np.random.default_rng(seed)
    nlist = len(sizes)
    lists = rng.permutation(np.repeat(np.arange(nlist), sizes)).astype(np.int32)
    n = len(lists)
    codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
    cb = (0.05 * rng.standard_normal((M, 256, CD // M))).astype(np.float32)
    c = rng.standard_normal((nlist, CD)).astype(np.float32)
    cent = (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float16)
    if ties:
        row = codes[0].copy()
        for size, copies in ((1000, 100), (257, 30)):
            members = np.flatnonzero(lists == sizes.index(size))
            codes[rng.choice(members, copies, replace=False)] = row
    return cent, cb, codes, lists


def _crafted(name):
    """(cent, cb, index with the threshold scan on, codes, lists) of a crafted index: 'fwd', 'rev' (the sizes reversed) or 'ties'."""
    from clip_retrieval_amd import knn

    key = ("crafted", name)
    if key not in _built:
        sizes = SIZES[::-1] if name == "rev" else SIZES
        cent, cb, codes, lists = _crafted_parts(sizes, {"fwd": 1, "rev": 2, "ties": 3}[name], name == "ties")
        ix = knn._ivfpq_from_codes(codes, lists, 0, cent, cb, M, 16, 0)  # pylint: disable=protected-access
        ix.pq_threshold_scan = True
        got, gl = ix.pq_codes()
        assert np.array_equal(got, codes) and np.array_equal(gl, lists) and np.array_equal(ix.pq_codebooks(), cb)
        _built[key] = (cent, cb, ix, codes, lists)
    return _built[key]


def _crafted_queries(B, seed):
    q = np.random.default_rng(seed).standard_normal((B, CD)).astype(np.float32)
    return np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True))


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for v in _built.values():
        v[3 if len(v) == 6 else 2].close()
    _built.clear()


# ------------------------------------------------------------------------------------------------ 1. encode
@pytest.mark.parametrize("d", [512, 768, 1024])
def test_encode_matches_numpy(d):
    """Device encode (the Lloyd step's assignment) at M = 256, ds = 2, 3, 4 = float64 argmin per sub-quantiser, modulo near-ties."""
    from clip_retrieval_amd.knn import PqBuilder

    n, nlist = 600, 5
    x = _data(n, d, d)
    rng = np.random.default_rng(d)
    cent = x[:nlist]
    lists = rng.integers(0, nlist, n).astype(np.int32)
    res = x.astype(np.float32) - cent[lists].astype(np.float32)
    cb = (0.05 * rng.standard_normal((M, 256, d // M))).astype(np.float32)
    b = PqBuilder(d, M)
    b.set_sample(x, lists, cent)
    b.set_codebooks(cb)
    sizes, codes = b.lloyd(want_codes=True)
    b.close()
    want, dist = _encode_in_chunks(res, cb)
    assert codes_match(codes, want, dist), f"d={d}: {(codes != want).sum()} codes differ beyond near-ties"
    for m in (0, 127, 128, 255):
        assert np.array_equal(sizes[m], np.bincount(codes[:, m], minlength=256))


# ------------------------------------------------------------------------------------------------ 2. search parity on built indexes
CASES = [(512, 8, 33, 40), (768, 1, 1, 64), (768, 80, 256, 40), (768, 96, 31, 1), (1024, 8, 300, 64), (1024, 80, 1, 40), (512, 96, 256, 64)]


@pytest.mark.parametrize("d,nprobe,B,k", CASES)
def test_search_parity(d, nprobe, B, k):
    x, cent, cb, ix, codes, lists = _index(d)
    assert ix.pq_m == M and ix.ntotal == 5000 and ix.nlist == 96 and codes.shape == (5000, M)
    assert np.array_equal(ix.pq_codebooks(), cb) and np.array_equal(lists, ix.ivf_lists)
    ix.nprobe = nprobe
    q = _queries(B, d, seed=B + k, x=x)
    D, I = ix.search(q, k)
    Do, Io, amb = np_adc_search(q, cent, cb, codes, lists, 0, nprobe, k)
    assert amb.mean() <= 0.10
    _check(D, I, Do, Io, amb, f"d={d} nprobe={nprobe} B={B} k={k}")


def test_codes_equal_numpy_encoding():
    """The built index's codes are the numpy encoding of its rows against their lists (modulo near-ties), d = 768 (ds = 3)."""
    x, cent, cb, ix, codes, lists = _index(768)
    res = x.astype(np.float32) - cent[lists].astype(np.float32)
    want = np_pq_encode(res, cb)
    bad = np.flatnonzero((codes != want).any(1))
    assert len(bad) <= 600  # the full distance array is formed for the rows that differ only
    if len(bad):
        w2, dist = _encode_in_chunks(res[bad], cb)
        assert codes_match(codes[bad], w2, dist), f"{len(bad)} rows differ beyond near-ties"


# ------------------------------------------------------------------------------------------------ 3. crafted lists
@pytest.mark.parametrize("B", [1, 33, 256])
@pytest.mark.parametrize("nprobe", [1, 5, 16])
@pytest.mark.parametrize("name", ["fwd", "rev"])
def test_crafted_lists(name, nprobe, B):
    """Offsets past empty lists, tails of every length, the multi-step walk of a 1 000-row list; B = 1 splits one query into the most
    shares."""
    cent, cb, ix, codes, lists = _crafted(name)
    ix.nprobe = nprobe
    q = _crafted_queries(B, 100 * nprobe + B)
    D, I = ix.search(q, 64)
    Do, Io, amb = np_adc_search(q, cent, cb, codes, lists, 0, nprobe, 64)
    assert amb.mean() <= 0.10
    _check(D, I, Do, Io, amb, f"{name} nprobe={nprobe} B={B}")
    assert nprobe < 16 or (I >= 0).all()


# ------------------------------------------------------------------------------------------------ 4. ties
@pytest.mark.parametrize("size,copies", [(1000, 100), (257, 30)])
def test_ties_go_to_the_lowest_ids(size, copies):
    """The copies of one code row in one list have the same score bit for bit: the run of equal D has ascending ids and is the
    restatement's (score descending, id ascending) order."""
    cent, cb, ix, codes, lists = _crafted("ties")
    l = SIZES.index(size)
    dec = cb[np.arange(M), codes[0]].reshape(-1)
    q = cent[l].astype(np.float32) + 4.0 * dec  # the query's own list holds the copies, and they are its best rows
    q = np.ascontiguousarray((q / np.linalg.norm(q))[None, :])
    for nprobe in (1, 16):
        ix.nprobe = nprobe
        D, I = ix.search(q, 64)
        Do, Io, amb = np_adc_search(q, cent, cb, codes, lists, 0, nprobe, 64)
        assert not amb.any()
        _check(D, I, Do, Io, amb, f"ties {size} nprobe={nprobe}")
        tied = np.flatnonzero((codes[I[0]] == codes[0]).all(1) & (lists[I[0]] == l))
        assert len(tied) == min(copies, 64) and tied[0] == 0 and (np.diff(tied) == 1).all(), tied  # the copies lead the result
        assert len(set(_bits(D[0, tied]).tolist())) == 1
        for a in range(64):  # every run of equal D, not only this one
            if a and D[0, a] == D[0, a - 1]:
                assert I[0, a] > I[0, a - 1]
        assert np.array_equal(I[0, tied], Io[0, tied])


# ------------------------------------------------------------------------------------------------ 5. sub-groups
SLAB_BYTES = sum(SIZES) * 4  # S x 4 at nprobe 16: every list is probed


@pytest.mark.parametrize("budget,groups", [(60 * SLAB_BYTES + 100, 5), (1, 256)])
def test_sub_groups_do_not_change_a_bit(monkeypatch, budget, groups):
    """KNNX_PQ_PARTIAL_MAX_BYTES read when the index becomes IVF-PQ: 256 queries in 5 sub-groups (60 + 60 + 60 + 60 + 16) and one by
    one give the D bits and ids of the index built without the variable, at k = 64 and through the threshold scan at k = 300."""
    from clip_retrieval_amd import knn

    assert -(-256 // max(1, budget // SLAB_BYTES)) == groups
    cent, cb, ix0, codes, lists = _crafted("fwd")
    ix0.nprobe = 16
    q = _crafted_queries(256, 77)
    D0, I0 = ix0.search(q, 64)
    E0, J0 = ix0.search(q, 300)
    l0, R0, K0 = ix0.range_search(q[:40], float(np.median(E0[:, 150])))
    monkeypatch.setenv("KNNX_PQ_PARTIAL_MAX_BYTES", str(budget))
    ix = knn._ivfpq_from_codes(codes, lists, 0, cent, cb, M, 16, 0)  # pylint: disable=protected-access
    monkeypatch.delenv("KNNX_PQ_PARTIAL_MAX_BYTES")
    try:
        ix.pq_threshold_scan = True
        D, I = ix.search(q, 64)
        assert np.array_equal(I, I0) and np.array_equal(_bits(D), _bits(D0))
        E, J = ix.search(q, 300)
        assert np.array_equal(J, J0) and np.array_equal(_bits(E), _bits(E0))
        l1, R1, K1 = ix.range_search(q[:40], float(np.median(E0[:, 150])))
        assert np.array_equal(l1, l0) and np.array_equal(K1, K0) and np.array_equal(_bits(R1), _bits(R0))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 6. same bits everywhere
def test_entry_points_agree_with_batched_search():
    """A query alone, as row 17 of a batch of 256, through search_device, search_dedup and 8 concurrent coalesced threads."""
    import torch

    x, cent, cb, ix, codes, lists = _index(768)
    ix.nprobe = 8
    q = _queries(256, 768, 2, x)
    D, I = ix.search(q, 40)
    D1, I1 = ix.search(q[17:18], 40)
    assert np.array_equal(I1[0], I[17]) and np.array_equal(_bits(D1[0]), _bits(D[17]))
    outs = [None] * 8

    def one(i):
        outs[i] = ix.search(q[i:i + 1], 40)

    th = [threading.Thread(target=one, args=(i,)) for i in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert np.array_equal(np.concatenate([o[1] for o in outs]), I[:8])
    assert np.array_equal(_bits(np.concatenate([o[0] for o in outs])), _bits(D[:8]))
    qd = torch.from_numpy(q).cuda()
    Dd = torch.empty((256, 40), dtype=torch.float32, device="cuda")
    Id = torch.empty((256, 40), dtype=torch.int64, device="cuda")
    ix.search_device(qd.data_ptr(), 256, 40, Dd.data_ptr(), Id.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(Id.cpu().numpy(), I) and np.array_equal(_bits(Dd.cpu().numpy()), _bits(D))
    for i in (0, 17):
        D2, I2, R2, _ = ix.search_dedup(q[i:i + 1], 40, want_r=True)
        assert np.array_equal(I2[0], I[i]) and np.array_equal(_bits(D2[0]), _bits(D[i]))
        assert np.array_equal(R2[0], ix.reconstruct_batch(I[i]))


# ------------------------------------------------------------------------------------------------ 7. threshold scan
def _threshold_case(which):
    if which == "crafted":
        cent, cb, ix, codes, lists = _crafted("fwd")
        return cent, cb, ix, codes, lists, 16, _crafted_queries(33, 5)
    x, cent, cb, ix, codes, lists = _index(768)
    ix.pq_threshold_scan = True
    return cent, cb, ix, codes, lists, 80, _queries(33, 768, 5, x)


@pytest.mark.parametrize("which", ["crafted", "built"])
def test_large_k(which):
    cent, cb, ix, codes, lists, nprobe, q = _threshold_case(which)
    ix.nprobe = nprobe
    n = len(lists)
    D64, I64 = ix.search(q, 64)
    for k in (65, 300, n + 10):
        D, I = ix.search(q, k)
        Do, Io, amb = np_adc_search(q, cent, cb, codes, lists, 0, nprobe, k)
        assert amb.mean() <= 0.10
        _check(D, I, Do, Io, amb, f"{which} k={k}")
        assert np.array_equal(I[:, :64], I64) and np.array_equal(_bits(D[:, :64]), _bits(D64)), k
    D1, I1 = ix.search(q[17:18], 300)
    D, I = ix.search(q, 300)
    assert np.array_equal(I1[0], I[17]) and np.array_equal(_bits(D1[0]), _bits(D[17]))


@pytest.mark.parametrize("which", ["crafted", "built"])
def test_range_search(which):
    """A threshold between the 1 999th and 2 000th score of the query that has the most rows above it: 1 .. 2 000 hits per query."""
    cent, cb, ix, codes, lists, nprobe, q = _threshold_case(which)
    ix.nprobe = nprobe
    parts, amb = np_adc_parts(q, cent, cb, codes, lists, 0, nprobe)
    top = [np.sort(S)[::-1] for _, S in parts]
    j = int(np.argmax([s[1999] for s in top]))
    thr = float(0.5 * (top[j][1998] + top[j][1999]))
    hits = [int((S > thr).sum()) for _, S in parts]
    assert 1 <= min(hits) and max(hits) <= 2000, (min(hits), max(hits))
    lims, D, I = ix.range_search(q, thr)
    worst, band = check_range(lims, D, I, parts, amb, thr, f"{which} thr={thr}")
    print(f"{which}: {int(lims[-1])} hits ({min(hits)} .. {max(hits)} per query), max |D - S| = {worst:.2e}, rows within the band {band}")


# ------------------------------------------------------------------------------------------------ 8. refine
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("kf", [1, 8])
def test_refine(kf, B):
    """kc = 64 (the top-k scan's queues feed the re-rank) and kc = 512 (the workgroup queue and the LDS selection), d = 1024."""
    from test_ivfpq_refine_gpu import _small_index as _refine_index

    key = ("refine", 1024)
    if key not in _built:
        x, cent, cb, ix = _refine_index(5000, 1024, 96, M, 8, seed=1024 + M)
        _built[key] = (x, cent, cb, ix, *ix.pq_codes())
    x, cent, cb, ix, codes, lists = _built[key]
    ix.k_factor = kf
    assert ix.pq_refine and ix.k_factor == kf and ix.pq_m == M
    k, nprobe = 64, 8
    q = _queries(B, 1024, seed=B + kf, x=x)
    parts, amb = np_refine_parts(q, x, cent, cb, codes, lists, 0, nprobe)
    assert amb.mean() <= 0.10
    D, I = ix.search(q, k)
    worst = check_refine(D, I, parts, amb, k, k * kf, f"refine kf={kf} B={B}")
    Ds, Is = np_refine_search(parts, k, k * kf)
    ok = ~amb
    assert np.array_equal(I[ok] >= 0, Is[ok] >= 0)
    assert not topk_sets_equal(I[ok], D[ok], Is[ok], Ds[ok].astype(np.float32), tol=REFINE_TOL)
    print(f"refine kf={kf} B={B}: max |D - E| = {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 9. rotation
def test_rotated_index():
    """OPQ256_768 ... PQ256x8 without the HNSW: parity in the rotated space, reconstruct in the original one."""
    from test_opq_gpu import _rotated_index

    n, d, nlist, nprobe = 3000, 768, 32, 8
    x, y, A, cent, cb, ix = _rotated_index(n, d, nlist, M, nprobe, seed=5)
    try:
        codes, lists = ix.pq_codes()
        q = _queries(33, d, seed=2, x=x)
        qr = (q.astype(np.float64) @ A.astype(np.float64).T).astype(np.float32)
        D, I, R = ix.search_and_reconstruct(q, 40)
        Do, Io, amb = np_adc_search(qr, cent, cb, codes, lists, 0, nprobe, 40)
        assert amb.mean() <= 0.10
        _check(D, I, Do, Io, amb, "rotated")
        assert (I >= 0).all()
        ids = I.reshape(-1)
        dec = cb[np.arange(M)[None, :], codes[ids]].reshape(len(ids), d).astype(np.float64)
        want = (cent[lists[ids]].astype(np.float64) + dec) @ A.astype(np.float64)  # A^T applied to the decoded rows
        assert R.shape == (33, 40, d) and np.abs(R.reshape(-1, d) - want).max() <= 1e-5
        assert np.array_equal(_bits(ix.reconstruct_batch(ids)), _bits(R.reshape(-1, d)))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 10. round trips
def test_reconstruct_is_the_decoded_vector():
    x, cent, cb, ix, codes, lists = _index(768)
    ids = np.array([0, 17, 4999, 1234, -1], dtype=np.int64)
    R = ix.reconstruct_batch(ids)
    for r, i in zip(R, ids):
        if i < 0:
            assert np.array_equal(r.view(np.uint32), np.full(768, 0xFFFFFFFF, np.uint32))
            continue
        assert np.array_equal(r, cent[lists[i]].astype(np.float32) + cb[np.arange(M), codes[i]].reshape(-1))


def test_save_load_round_trip(tmp_path):
    from clip_retrieval_amd import knn

    x, cent, cb, ix, codes, lists = _index(512)
    ix.nprobe = 8
    q = _queries(40, 512, 5, x)
    D0, I0 = ix.search(q, 40)
    out = str(tmp_path / "idx")
    knn.save_index(ix, out)
    loaded = knn.load_index(out)
    try:
        assert loaded.pq_m == M and loaded.nprobe == 8
        c1, l1 = loaded.pq_codes()
        assert np.array_equal(c1, codes) and np.array_equal(l1, lists) and np.array_equal(loaded.pq_codebooks(), cb)
        D1, I1 = loaded.search(q, 40)
        assert np.array_equal(I0, I1) and np.array_equal(_bits(D0), _bits(D1))
    finally:
        loaded.close()


def test_two_shards_on_one_gpu():
    from clip_retrieval_amd.knn import ShardedMi355xIndex, build_ivfpq_index

    x, cent, cb, ix, codes, lists = _index(768)
    ix.nprobe = 8
    cut = [0, 2100, 5000]
    shards = [build_ivfpq_index(x[cut[g]:cut[g + 1]], 96, M, nprobe=8, id_base=cut[g], centroids=cent, codebooks=cb) for g in range(2)]
    assert np.array_equal(np.concatenate([s.pq_codes()[0] for s in shards]), codes)
    sh = ShardedMi355xIndex.from_shards(shards, cut[:2])
    try:
        q = _queries(33, 768, 4, x)
        D0, I0 = ix.search(q, 40)
        D, I = sh.search(q, 40)
        assert np.array_equal(I, I0) and np.array_equal(_bits(D), _bits(D0))
    finally:
        sh.close()


def test_device_build_equals_host_build():
    import torch

    from clip_retrieval_amd.knn import build_ivfpq_index_device

    x, cent, cb, ix, codes, lists = _index(768)
    xd = torch.from_numpy(x).cuda()

    def fill_rows(dst, row0, count, stride):  # device rows -> dst, completed on return
        src = xd[row0:row0 + count * stride:stride][:count].contiguous()
        torch.cuda.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src.data_ptr()), src.numel() * 2, 3) == 0  # device to device
        torch.cuda.synchronize()  # (a device-to-device hipMemcpy does not wait on the host: without this the copy is not "completed on return")

    dev, stats = build_ivfpq_index_device(fill_rows, 5000, 768, 96, M, nprobe=8, centroids=cent, codebooks=cb, chunk=3000)
    try:
        c1, l1 = dev.pq_codes()
        assert np.array_equal(l1, lists) and np.array_equal(c1, codes)
        assert stats["bytes_per_row"] == M + 12
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ 11. quality
def test_m256_reconstructs_and_recalls_better_than_m64():
    """Device-trained M = 64 and M = 256 on the 6 000 x 512 mixture corpus, same coarse centroids, nprobe = nlist.  numpy PQ on the same
    corpus: reconstruction error 0.254 (M = 64) against 0.0083 (M = 256), recall@10 0.70 against 0.92."""
    from clip_retrieval_amd.knn import IvfBuilder, PqBuilder, build_ivfpq_index, train_ivf_centroids, train_pq_codebooks

    n, d, nlist, nc = 6000, 512, 16, 40
    x = synth_mixture_rows(np.arange(n), d, 7, nc)
    cent = train_ivf_centroids(x, nlist, niter=4, seed=0)
    b = IvfBuilder(d, nlist)
    b.set_centroids(cent)
    lists = b.assign(x)
    b.close()
    res = x.astype(np.float32) - cent[lists].astype(np.float32)
    q = _queries(64, d, 8, x)
    exact = np.argsort(-(q @ x.astype(np.float32).T), axis=1)[:, :10]
    err, rec = {}, {}
    for m in (64, M):
        pb = PqBuilder(d, m)
        pb.set_sample(x, lists, cent)
        cb = train_pq_codebooks(pb, niter=6, seed=3)
        pb.close()
        ix = build_ivfpq_index(x, nlist, m, nprobe=nlist, centroids=cent, codebooks=cb)
        codes, _ = ix.pq_codes()
        dec = cb[np.arange(m)[None, :], codes].reshape(n, d)
        err[m] = float(((res - dec) ** 2).sum(1).mean())
        _, I = ix.search(q, 10)
        ix.close()
        rec[m] = float(np.mean([len(set(a) & set(e)) / 10 for a, e in zip(I, exact)]))
    print(f"reconstruction error {err}, recall@10 {rec}")
    assert err[M] < err[64]
    assert rec[M] >= rec[64]


# ------------------------------------------------------------------------------------------------ 12. refusals
@pytest.mark.parametrize("d,m", [(256, 256), (512, 24), (512, 512)])
def test_refusals(d, m):
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import Mi355xIndex, PqBuilder

    e = Mi355xIndex(d)
    try:
        lib, h = e._lib, e._h  # pylint: disable=protected-access
        cb = np.zeros(256 * d, np.float32)
        assert lib.knnx_ivfpq_set_quantizer(h, m, cb.ctypes.data) == KNNX_E_ARG
        msg = lib.knnx_last_error().decode()
        assert "M in {16, 32, 64, 128} dividing d" in msg and "M = 256 with d >= 512" in msg
        with pytest.raises(HipLibraryError, match=r"M in \{16, 32, 64, 128\} dividing d.*M = 256 with d >= 512"):
            e.set_pq_quantizer(m, cb)
    finally:
        e.close()
    with pytest.raises(HipLibraryError, match=r"M in \{16, 32, 64, 128\} dividing d.*M = 256 with d >= 512"):
        PqBuilder(d, m)
