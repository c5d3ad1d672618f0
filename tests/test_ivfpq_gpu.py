"""IVF-PQ (faiss IndexIVFPQ(IndexFlatIP(d), d, nlist, M, 8), inner product, by_residual) against a numpy restatement built from the
index's own centroids, codebooks and codes: encoding, the codebook Lloyd step, ADC search, decoding, the other entry points, shards,
save / load, the device-streamed build, refusals and training quality."""
import os
import shutil
import threading

import numpy as np
import pytest

from oracle.knn_oracle import synth_mixture_rows, topk_sets_equal

NEG = np.float32(-3.4028234663852886e38)
pytestmark = pytest.mark.gpu


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float16)


def _queries(nq, d, seed, x):
    rng = np.random.default_rng(seed)
    q = x[rng.integers(0, len(x), nq)].astype(np.float32) + 0.3 * rng.standard_normal((nq, d)).astype(np.float32) / np.sqrt(d)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32)


# ------------------------------------------------------------------------------------------------ numpy restatement
def np_encode(res, cb):
    """res f32 [n, d] residuals, cb f32 [M, 256, ds] -> (codes [n, M], squared distances float64 [n, M, 256])."""
    M, _, ds = cb.shape
    r = res.astype(np.float64).reshape(res.shape[0], M, ds)
    dist = ((r[:, :, None, :] - cb.astype(np.float64)[None]) ** 2).sum(-1)
    return dist.argmin(-1).astype(np.uint8), dist


def codes_match(got, want, dist, rel=1e-5):
    """Codes equal except where the two squared distances are within `rel` of each other."""
    bad = got != want
    if not bad.any():
        return True
    n, m = np.nonzero(bad)
    a, b = dist[n, m, got[bad]], dist[n, m, want[bad]]
    return bool((np.abs(a - b) <= rel * np.maximum(np.abs(b), 1e-30)).all())


def np_adc_search(q, cent, cb, codes, lists, id_base, nprobe, k):
    """D, I of faiss IndexIVFPQ.search (float64), plus a mask of queries whose probe set is ambiguous (the nprobe-th and next coarse
    scores within 1e-6)."""
    M, _, ds = cb.shape
    nlist = cent.shape[0]
    qd = q.astype(np.float64)
    cs = qd @ cent.astype(np.float32).astype(np.float64).T
    lut = np.einsum("qmt,mjt->qmj", qd.reshape(q.shape[0], M, ds), cb.astype(np.float64))
    n = q.shape[0]
    D = np.full((n, k), NEG, dtype=np.float64)
    I = np.full((n, k), -1, dtype=np.int64)
    amb = np.zeros(n, dtype=bool)
    for i in range(n):
        order = np.lexsort((np.arange(nlist), -cs[i]))
        np_ = min(nprobe, nlist)
        if np_ < nlist and abs(cs[i, order[np_ - 1]] - cs[i, order[np_]]) <= 1e-6:
            amb[i] = True
        rows = np.flatnonzero(np.isin(lists, order[:np_]))
        s = cs[i, lists[rows]] + lut[i][np.arange(M)[None, :], codes[rows]].sum(1)
        top = np.lexsort((rows, -s))[:k]
        D[i, :len(top)] = s[top]
        I[i, :len(top)] = rows[top] + id_base
    return D, I, amb


def _check(D, I, Do, Io, amb, ctx):
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == Do.shape, ctx
    ok = ~amb
    D, I, Do, Io = D[ok], I[ok], Do[ok], Io[ok]
    assert np.array_equal(I >= 0, Io >= 0), f"{ctx}: -1 padding differs"
    assert (D[I < 0] == NEG).all(), f"{ctx}: padding score"
    v = Io >= 0
    err = np.abs(D[v].astype(np.float64) - Do[v])
    assert err.max(initial=0) <= 1e-5, f"{ctx}: max score err {err.max()}"
    for i in range(D.shape[0]):
        dv = D[i][I[i] >= 0]
        assert (np.diff(dv) <= 0).all(), f"{ctx}: query {i} not sorted"
    bad = topk_sets_equal(I, D, Io, Do.astype(np.float32), tol=1e-5)
    assert not bad, f"{ctx}: id sets differ beyond near-ties: {bad[:3]}"


def _seed_codebooks(x, cent, lists, M, seed):
    """Codebooks from residual sub-vectors of random rows (any codebook is a valid quantizer; training is tested separately)."""
    rng = np.random.default_rng(seed)
    res = x.astype(np.float32) - cent[lists].astype(np.float32)
    d = x.shape[1]
    ds = d // M
    cb = np.empty((M, 256, ds), np.float32)
    for m in range(M):
        cb[m] = res[rng.choice(len(x), 256, replace=False), m * ds:(m + 1) * ds]
    return cb


def _small_index(n, d, nlist, M, nprobe, seed):
    from clip_retrieval_amd.knn import IvfBuilder, build_ivfpq_index

    x = _data(n, d, seed)
    rng = np.random.default_rng(seed + 1)
    cent = x[rng.choice(n, nlist, replace=False)]
    b = IvfBuilder(d, nlist)
    b.set_centroids(cent)
    lists = b.assign(x)
    b.close()
    cb = _seed_codebooks(x, cent, lists, M, seed + 2)
    ix = build_ivfpq_index(x, nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb)
    return x, cent, cb, ix


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("d", [512, 768, 1024])
def test_encode_matches_numpy(d):
    """Device encode (the Lloyd step's assignment) = float64 argmin per sub-quantiser, for every M, modulo near-ties."""
    from clip_retrieval_amd.knn import PqBuilder

    n, nlist = 600, 5
    x = _data(n, d, d)
    rng = np.random.default_rng(d)
    cent = x[:nlist]
    lists = rng.integers(0, nlist, n).astype(np.int32)
    res = x.astype(np.float32) - cent[lists].astype(np.float32)
    for M in (16, 32, 64, 128):
        cb = (0.05 * rng.standard_normal((M, 256, d // M))).astype(np.float32)
        b = PqBuilder(d, M)
        b.set_sample(x, lists, cent)
        b.set_codebooks(cb)
        _, codes = b.lloyd(want_codes=True)
        b.close()
        want, dist = np_encode(res, cb)
        assert codes_match(codes, want, dist), f"d={d} M={M}: {(codes != want).sum()} codes differ beyond near-ties"


def test_pq_lloyd_iteration_matches_numpy():
    """One device PQ Lloyd iteration = one numpy iteration from the same initial codebooks."""
    from clip_retrieval_amd.knn import PqBuilder

    n, d, M, nlist = 3000, 768, 32, 6
    x = _data(n, d, 3)
    rng = np.random.default_rng(3)
    cent = x[:nlist]
    lists = rng.integers(0, nlist, n).astype(np.int32)
    res = x.astype(np.float32) - cent[lists].astype(np.float32)
    cb0 = _seed_codebooks(x, cent, lists, M, 4)
    b = PqBuilder(d, M)
    b.set_sample(x, lists, cent)
    b.set_codebooks(cb0)
    sizes, codes = b.lloyd(want_codes=True)
    cb1 = b.codebooks()
    b.close()
    want, dist = np_encode(res, cb0)
    assert codes_match(codes, want, dist)
    ds = d // M
    r = res.reshape(n, M, ds).astype(np.float64)
    for m in range(M):
        assert np.array_equal(sizes[m], np.bincount(codes[:, m], minlength=256))
        for j in range(256):
            mem = codes[:, m] == j
            expect = r[mem, m].mean(0) if mem.any() else cb0[m, j]
            assert np.allclose(cb1[m, j], expect, rtol=0, atol=1e-5), f"m={m} j={j}"


# ------------------------------------------------------------------------------------------------ search parity
# (d, M, nprobe, B, k): every value of d {512, 768, 1024}, M {16, 32, 64, 128}, nprobe {1, 8, 80, nlist}, B {1, 31, 33, 256, 300},
# k {1, 40, 64} appears at least once
CASES = [(512, 16, 8, 33, 40), (512, 128, 1, 1, 64), (768, 32, 80, 31, 1), (768, 64, "nlist", 256, 40), (1024, 64, 8, 300, 64),
         (1024, 128, 80, 1, 40), (768, 16, 1, 256, 64), (1024, 32, "nlist", 33, 1), (512, 64, 80, 300, 40), (768, 128, 8, 31, 64)]


@pytest.mark.parametrize("d,M,nprobe,B,k", CASES)
def test_search_parity(d, M, nprobe, B, k):
    n, nlist = 5000, 96
    nprobe = nlist if nprobe == "nlist" else nprobe
    x, cent, cb, ix = _small_index(n, d, nlist, M, nprobe, seed=d + M)
    assert ix.pq_m == M and ix.ntotal == n and ix.nlist == nlist
    assert np.array_equal(ix.pq_codebooks(), cb)
    codes, lists = ix.pq_codes()
    assert np.array_equal(lists, ix.ivf_lists)
    q = _queries(B, d, seed=B + k, x=x)
    D, I = ix.search(q, k)
    Do, Io, amb = np_adc_search(q, cent, cb, codes, lists, 0, nprobe, k)
    assert amb.mean() < 0.5
    _check(D, I, Do, Io, amb, f"d={d} M={M} nprobe={nprobe} B={B} k={k}")
    ix.close()


def test_codes_equal_numpy_encoding():
    """The index's codes are the numpy encoding of its input rows against their lists (modulo near-ties)."""
    for d, M in ((768, 64), (512, 128)):
        x, cent, cb, ix = _small_index(2000, d, 16, M, 4, seed=11)
        codes, lists = ix.pq_codes()
        want, dist = np_encode(x.astype(np.float32) - cent[lists].astype(np.float32), cb)
        assert codes_match(codes, want, dist), f"d={d} M={M}"
        ix.close()


def test_reconstruct_is_the_decoded_vector():
    x, cent, cb, ix = _small_index(3000, 768, 32, 64, 8, seed=5)
    codes, lists = ix.pq_codes()
    ids = np.array([0, 17, 2999, 1234, -1], dtype=np.int64)
    R = ix.reconstruct_batch(ids)
    M, ds = 64, 768 // 64
    for r, i in zip(R, ids):
        if i < 0:
            assert np.array_equal(r.view(np.uint32), np.full(768, 0xFFFFFFFF, np.uint32))
            continue
        dec = cb[np.arange(M), codes[i]].reshape(-1)
        assert np.array_equal(r, cent[lists[i]].astype(np.float32) + dec)
    q = _queries(4, 768, 1, x)
    D, I, R = ix.search_and_reconstruct(q, 64)
    assert np.array_equal(R.view(np.uint32), ix.reconstruct_batch(I.reshape(-1)).reshape(R.shape).view(np.uint32))
    ix.close()


def test_entry_points_agree_with_batched_search():
    """Threaded single-query callers (the coalescer), search_device and search_dedup = the batched host search."""
    import torch

    x, _, _, ix = _small_index(4000, 512, 32, 32, 8, seed=9)
    q = _queries(48, 512, 2, x)
    D, I = ix.search(q, 40)
    outs = [None] * len(q)

    def one(i):
        outs[i] = ix.search(q[i:i + 1], 40)

    th = [threading.Thread(target=one, args=(i,)) for i in range(len(q))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert np.array_equal(np.concatenate([o[1] for o in outs]), I)
    assert np.array_equal(np.concatenate([o[0] for o in outs]), D)
    qd = torch.from_numpy(q).cuda()
    Dd = torch.empty((len(q), 40), dtype=torch.float32, device="cuda")
    Id = torch.empty((len(q), 40), dtype=torch.int64, device="cuda")
    ix.search_device(qd.data_ptr(), len(q), 40, Dd.data_ptr(), Id.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(Id.cpu().numpy(), I) and np.array_equal(Dd.cpu().numpy(), D)
    for i in range(3):
        D1, I1, R1, _ = ix.search_dedup(q[i:i + 1], 40, want_r=True)
        assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0], D[i])
        assert np.array_equal(R1[0], ix.reconstruct_batch(I[i]))
    ix.close()


def test_two_shards_on_one_gpu():
    from clip_retrieval_amd.knn import IvfBuilder, ShardedMi355xIndex, build_ivfpq_index

    n, d, nlist, M, nprobe = 6000, 768, 48, 32, 6
    x = _data(n, d, 21)
    cent = x[np.random.default_rng(2).choice(n, nlist, replace=False)]
    b = IvfBuilder(d, nlist)
    b.set_centroids(cent)
    lists = b.assign(x)
    b.close()
    cb = _seed_codebooks(x, cent, lists, M, 3)
    cut = [0, 2500, n]
    shards = [build_ivfpq_index(x[cut[g]:cut[g + 1]], nlist, M, nprobe=nprobe, id_base=cut[g], centroids=cent, codebooks=cb) for g in range(2)]
    codes = np.concatenate([s.pq_codes()[0] for s in shards])
    ix = ShardedMi355xIndex.from_shards(shards, cut[:2])
    q = _queries(20, d, 4, x)
    D, I = ix.search(q, 40)
    Do, Io, amb = np_adc_search(q, cent, cb, codes, lists, 0, nprobe, 40)
    _check(D, I, Do, Io, amb, "two shards")
    ix.close()


def test_save_delete_embeddings_load(tmp_path):
    """An IVF-PQ folder is self-contained: built from a folder of embeddings, saved, embeddings deleted, loaded: identical D and I."""
    from clip_retrieval_amd import knn

    n, d, nlist, M = 5000, 512, 32, 64
    emb = tmp_path / "emb"
    emb.mkdir()
    x = _data(n, d, 31)
    np.save(emb / "img_emb_0.npy", x[:3000])
    np.save(emb / "img_emb_1.npy", x[3000:])
    built = knn.build_ivfpq_index_from_folder(str(emb), nlist, M, nprobe=8, niter=3, pq_niter=3, chunk=2048)
    q = _queries(40, d, 5, x)
    D0, I0 = built.search(q, 40)
    out = str(tmp_path / "idx")
    knn.save_index(built, out)
    built.close()
    shutil.rmtree(emb)
    assert sorted(os.listdir(out)) == sorted(["ivf_pq_centroids.npy", "ivf_pq_codebooks.npy", "ivf_pq_codes.npy", "ivf_pq_lists.npy",
                                              knn.IVFPQ_MANIFEST])
    loaded = knn.load_index(out)
    assert loaded.pq_m == M and loaded.nprobe == 8
    D1, I1 = loaded.search(q, 40)
    assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
    loaded.close()
    sharded = knn.load_index(out, devices=[0, 0])
    D2, I2 = sharded.search(q, 40)
    assert np.array_equal(I0, I2) and np.array_equal(D0, D2)
    sharded.close()


def test_device_build_equals_host_build():
    import ctypes as C

    import torch

    from clip_retrieval_amd.knn import build_ivfpq_index, build_ivfpq_index_device

    n, d, nlist, M = 7000, 768, 24, 64
    x, cent, cb, host = _small_index(n, d, nlist, M, 4, seed=41)
    xd = torch.from_numpy(x).cuda()

    def fill_rows(dst, row0, count, stride):  # device rows -> dst, completed on return
        src = xd[row0:row0 + count * stride:stride][:count].contiguous()
        torch.cuda.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src.data_ptr()), src.numel() * 2, 3) == 0  # device to device
        torch.cuda.synchronize()  # (a device-to-device hipMemcpy does not wait on the host: without this the copy is not "completed on return")

    dev, stats = build_ivfpq_index_device(fill_rows, n, d, nlist, M, nprobe=4, centroids=cent, codebooks=cb, chunk=3000)
    c0, l0 = host.pq_codes()
    c1, l1 = dev.pq_codes()
    assert np.array_equal(l0, l1) and np.array_equal(c0, c1)
    assert stats["bytes_per_row"] == M + 12
    host.close()
    dev.close()


def test_refusals():
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import Mi355xIndex

    x, _, _, ix = _small_index(1000, 512, 8, 16, 2, seed=1)
    q = _queries(2, 512, 1, x)
    with pytest.raises(HipLibraryError, match="k > 64 is not supported on an IVF-PQ index"):
        ix.search(q, 65)
    with pytest.raises(HipLibraryError, match="range_search is not supported on an IVF-PQ index"):
        ix.range_search(q, 0.5)
    with pytest.raises(HipLibraryError, match="IVF-PQ"):
        ix.add(x[:3])
    with pytest.raises(HipLibraryError, match="IVF-PQ"):
        ix.reset()
    ix.close()
    e = Mi355xIndex(512)
    with pytest.raises(HipLibraryError, match=r"M in \{16, 32, 64, 128\} dividing d"):
        e.set_pq_quantizer(24, np.zeros(256 * 512, np.float32))
    e.close()


def test_training_quality():
    """Recall@10 at nprobe = nlist within 0.03 of a numpy-trained IVF-PQ (same coarse centroids, sample and seeds); the trained
    codebooks reconstruct better than the initial ones."""
    from clip_retrieval_amd.knn import IvfBuilder, PqBuilder, build_ivfpq_index, train_ivf_centroids, train_pq_codebooks

    n, d, nlist, M, nc = 6000, 512, 16, 32, 40
    x = synth_mixture_rows(np.arange(n), d, 7, nc)
    cent = train_ivf_centroids(x, nlist, niter=4, seed=0)
    b = IvfBuilder(d, nlist)
    b.set_centroids(cent)
    lists = b.assign(x)
    b.close()
    res = x.astype(np.float32) - cent[lists].astype(np.float32)
    pb = PqBuilder(d, M)
    pb.set_sample(x, lists, cent)
    cb_dev = train_pq_codebooks(pb, niter=6, seed=3)
    pb.close()
    # numpy: the same initial rows (train_pq_codebooks' draw), the same iterations
    rng = np.random.default_rng(3)
    rows = np.concatenate([np.sort(rng.choice(n, 256, replace=False)) for _ in range(M)]).reshape(M, 256)
    ds = d // M
    cb0 = np.stack([res[rows[m], m * ds:(m + 1) * ds] for m in range(M)]).astype(np.float32)
    cb_np = cb0.astype(np.float64)
    for it in range(6):
        codes, _ = np_encode(res, cb_np)
        r = res.reshape(n, M, ds).astype(np.float64)
        for m in range(M):
            cnt = np.bincount(codes[:, m], minlength=256)
            s = np.zeros((256, ds))
            np.add.at(s, codes[:, m], r[:, m])
            nz = cnt > 0
            cb_np[m, nz] = s[nz] / cnt[nz, None]
            if it < 5 and (~nz).any():
                cb_np[m, ~nz] = r[rng.choice(n, (~nz).sum()), m]
    cb_np = cb_np.astype(np.float32)

    def err(cb):
        c, _ = np_encode(res, cb)
        dec = cb[np.arange(M)[None, :], c].reshape(n, d)
        return float(((res - dec) ** 2).sum(1).mean())

    assert err(cb_dev) < err(cb0)
    q = _queries(64, d, 8, x)
    exact = np.argsort(-(q @ x.astype(np.float32).T), axis=1)[:, :10]

    def recall(cb):
        ix = build_ivfpq_index(x, nlist, M, nprobe=nlist, centroids=cent, codebooks=cb)
        _, I = ix.search(q, 10)
        ix.close()
        return np.mean([len(set(a) & set(b)) / 10 for a, b in zip(I, exact)])

    r_dev, r_np = recall(cb_dev), recall(cb_np)
    assert r_dev >= r_np - 0.03, (r_dev, r_np)
