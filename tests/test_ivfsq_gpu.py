"""IVF-SQ8 (faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_8bit), inner product, not residual) against the numpy
restatement of test_ivfsq_cpu.py: encoding and training bit for bit, search parity at the tile edges of the lists, batch independence,
padding, reconstruct / R / dedup bit for bit, IVF-Flat's ranking, shards, save / load, list-ordered ids, the hot path, refusals, and
that the IVF-Flat path next to it is untouched."""
import ctypes as C
import os
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from oracle.knn_oracle import synth_mixture_rows, topk_sets_equal
from test_ivfsq_cpu import (MIX_CLUSTERS, NEG, corpus, np_layout_old_to_new, np_ranges, np_sq_decode, np_sq_encode, np_sq_search,
                            top10_overlap)

pytestmark = pytest.mark.gpu

NLIST = 24
# rows per list: the tile edges 0, 1, 31, 32, 33, one list of several hundred rows, the rest ordinary
SIZES = np.array([0, 1, 31, 32, 33, 700, 64, 65, 96, 0, 5, 130, 17, 250, 2, 63, 40, 128, 90, 11, 160, 75, 1, 300], dtype=np.int64)
N = int(SIZES.sum())
DUP = (10, 11, 12, 13)  # rows that are near-copies of row 10 (dedup links)


def _queries(nq, d, seed, x):
    rng = np.random.default_rng(seed)
    q = x[rng.integers(0, len(x), nq)].astype(np.float32) + 0.3 * rng.standard_normal((nq, d)).astype(np.float32) / np.sqrt(d)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32)


def _crafted(d):
    """(x, lists, cent, (vmin, vdiff)): N rows with the list sizes above in shuffled order, centroids = the lists' normalised means
    (random unit vectors for the empty lists), ranges trained on every other row -- so rows fall outside them -- with one constant
    column (vdiff == 0) that the rows do vary in."""
    rng = np.random.default_rng(d)
    x = corpus("mixture" if d == 256 else "isotropic", d, N).copy()
    for r in DUP[1:]:
        x[r] = (x[DUP[0]].astype(np.float32) * (1 + 0.002 * (r - DUP[0]))).astype(np.float16)
    lists = np.repeat(np.arange(NLIST, dtype=np.int32), SIZES)
    rng.shuffle(lists)
    lists[list(DUP)] = int(np.argmax(SIZES))  # the near-copies share the long list
    lists = _fix_sizes(lists)
    cent = np.zeros((NLIST, d), np.float32)
    for l in range(NLIST):
        m = x[lists == l].astype(np.float32).mean(0) if (lists == l).any() else rng.standard_normal(d).astype(np.float32)
        cent[l] = m / np.linalg.norm(m)
    vmin, vdiff = np_ranges(x[::2])
    vdiff[7] = 0
    return x, lists, cent.astype(np.float16), (vmin, vdiff)


def _fix_sizes(lists):
    """Put the list sizes back to SIZES after rows were moved by hand (rows not in DUP change lists)."""
    have = np.bincount(lists, minlength=NLIST)
    free = [i for i in range(len(lists)) if i not in DUP]
    for l in np.flatnonzero(have < SIZES):
        for _ in range(int(SIZES[l] - have[l])):
            donor = next(i for i in free if have[lists[i]] > SIZES[lists[i]])
            have[lists[donor]] -= 1
            lists[donor] = l
            have[l] += 1
    assert np.array_equal(np.bincount(lists, minlength=NLIST), SIZES)
    return lists


_CACHE = {}


def _index(d):
    """The crafted index of width d, built once (host rows through knnx_ivf_add_assigned, in chunks that split lists)."""
    from clip_retrieval_amd import knn

    if d not in _CACHE:
        x, lists, cent, ranges = _crafted(d)
        ix = knn._ivfsq_encode_chunks(((o, x[o:o + 1000]) for o in range(0, N, 1000)), N, d, NLIST, cent, ranges, lists, 5, 0, 0)  # pylint: disable=protected-access
        codes = np_sq_encode(x, *ranges)
        _CACHE[d] = SimpleNamespace(x=x, lists=lists, cent=cent, ranges=ranges, ix=ix, codes=codes)
    return _CACHE[d]


def _check(D, I, Do, Io, amb, ctx, tol=1e-5):
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == Do.shape, ctx
    ok = ~amb
    D, I, Do, Io = D[ok], I[ok], Do[ok], Io[ok]
    assert np.array_equal(I >= 0, Io >= 0), f"{ctx}: -1 padding differs"
    assert (D[I < 0] == NEG).all(), f"{ctx}: padding score"
    v = Io >= 0
    err = np.abs(D[v].astype(np.float64) - Do[v])
    print(f"{ctx}: max score error {err.max(initial=0):.3e} over {int(v.sum())} results")
    assert err.max(initial=0) <= tol, f"{ctx}: max score err {err.max()}"
    for i in range(D.shape[0]):
        dv = D[i][I[i] >= 0]
        assert (np.diff(dv) <= 0).all(), f"{ctx}: query {i} not sorted"
    bad = topk_sets_equal(I, D, Io, Do.astype(np.float32), tol=tol)
    assert not bad, f"{ctx}: id sets differ beyond near-ties: {bad[:3]}"


# ------------------------------------------------------------------------------------------------ encode, codes in and out
@pytest.mark.parametrize("d", [256, 768, 1024])
def test_codes_are_the_numpy_encoding(d):
    """sq_codes() of rows that went through knnx_ivf_add_assigned = np.clip(np.floor((x - vmin) * scale), 0, 255), bit for bit --
    rows outside the trained range and a vdiff == 0 column among them; add_codes then get_codes round-trips."""
    from clip_retrieval_amd import knn

    c = _index(d)
    assert c.ix.is_sq and c.ix.ntotal == N and c.ix.nlist == NLIST and c.ix.pq_m == 0
    vmin, vdiff = c.ix.sq_quantizer()
    assert np.array_equal(vmin, c.ranges[0]) and np.array_equal(vdiff, c.ranges[1])
    codes, lists = c.ix.sq_codes()
    assert np.array_equal(lists, c.lists)
    assert (c.codes == 0).any() and (c.codes == 255).any() and (c.codes[:, 7] == 0).all()  # clamped rows exist; the constant column
    x32 = c.x.astype(np.float32)
    assert (x32 < vmin).any() and (x32 > vmin + vdiff).any()
    assert np.array_equal(codes, c.codes), f"{(codes != c.codes).sum()} code bytes differ"
    again = knn._ivfsq_from_codes(codes, lists, 0, c.cent, c.ranges, 5, 0, chunk=777)  # pylint: disable=protected-access
    codes2, lists2 = again.sq_codes()
    assert np.array_equal(codes2, codes) and np.array_equal(lists2, lists)
    q = _queries(9, d, 3, c.x)
    D0, I0 = c.ix.search(q, 40)
    D1, I1 = again.search(q, 40)
    assert np.array_equal(I0, I1) and np.array_equal(D0.view(np.uint32), D1.view(np.uint32))
    again.close()


def test_device_build_encodes_like_numpy():
    """knnx_ivf_add_assigned_device: rows that never leave the GPU get the same code bytes."""
    import torch

    from clip_retrieval_amd.knn import IvfBuilder, build_ivfsq_index_device

    c = _index(768)
    d = 768
    xd = torch.from_numpy(c.x).cuda()

    def fill_rows(dst, row0, count, stride):  # device rows -> dst, completed on return
        src = xd[row0:row0 + count * stride:stride][:count].contiguous()
        torch.cuda.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src.data_ptr()), src.numel() * 2, 3) == 0  # device to device
        torch.cuda.synchronize()  # (a device-to-device hipMemcpy does not wait on the host: without this the copy is not "completed on return")

    dev, stats = build_ivfsq_index_device(fill_rows, N, d, NLIST, nprobe=4, centroids=c.cent, ranges=c.ranges, chunk=1100, keep_lists=True)
    b = IvfBuilder(d, NLIST)
    b.set_centroids(c.cent)
    l0 = b.assign(c.x)
    b.close()
    c1, l1 = dev.sq_codes()
    assert np.array_equal(l0, l1) and np.array_equal(l1, dev.ivf_lists)
    assert np.array_equal(c1, c.codes)
    assert stats["bytes_per_row"] == d + 12
    # trained by default: the ranges are the sample's column min / max
    dev2, _ = build_ivfsq_index_device(fill_rows, N, d, NLIST, nprobe=4, centroids=c.cent, chunk=2000)
    vmin, vdiff = dev2.sq_quantizer()
    ns = min(N, NLIST * 64)  # the builder's strided training sample
    st = max(1, N // ns)
    want = np_ranges(c.x[0:ns * st:st][:ns])
    assert np.array_equal(vmin, want[0]) and np.array_equal(vdiff, want[1])
    dev.close()
    dev2.close()


@pytest.mark.parametrize("n,d", [(1037, 768), (64, 256), (4099, 1024), (130, 200)])
def test_column_min_max_is_numpys(n, d):
    """knnx_colminmax_device = x.astype(f32).min(0) / .max(0) bit for bit; n is no multiple of the 64 rows a workgroup folds at a time."""
    import torch

    from clip_retrieval_amd import load_library
    from clip_retrieval_amd.knn import train_sq_ranges

    rng = np.random.default_rng(n)
    x = (0.1 * rng.standard_normal((n, d))).astype(np.float16)
    x[n - 1, 3] = 9.0  # the extremes sit in the last, partial group of rows
    x[n - 1, 4] = -9.0
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    lib = load_library()
    vmin, vmax = np.empty(d, np.float32), np.empty(d, np.float32)
    assert lib.knnx_colminmax_device(0, C.c_void_p(xd.data_ptr()), n, d, vmin.ctypes.data, vmax.ctypes.data, None) == 0, lib.knnx_last_error()
    x32 = x.astype(np.float32)
    assert np.array_equal(vmin.view(np.uint32), x32.min(0).view(np.uint32)) and np.array_equal(vmax.view(np.uint32), x32.max(0).view(np.uint32))
    a, b = train_sq_ranges(x, chunk=500)  # host rows, chunked
    c, e = train_sq_ranges(xd.data_ptr(), n, d)  # device rows
    for got in ((a, b), (c, e)):
        assert np.array_equal(got[0], x32.min(0)) and np.array_equal(got[1], x32.max(0) - x32.min(0))


# ------------------------------------------------------------------------------------------------ search parity
# (d, nprobe, k, B): every d {256, 768, 1024}, nprobe {1, 5, 24}, k {1, 40, 64}, B {1, 32, 33, 300} appears
CASES = [(256, 1, 1, 1), (256, 5, 40, 33), (256, 24, 64, 300), (768, 5, 64, 32), (768, 24, 1, 33), (768, 1, 40, 300),
         (1024, 24, 40, 1), (1024, 1, 64, 32), (1024, 5, 1, 300), (1024, 24, 64, 33)]


@pytest.mark.parametrize("d,nprobe,k,B", CASES)
def test_search_parity(d, nprobe, k, B):
    """D, I against the float64 restatement on the index's own codes: padding, order, scores within the project's 1e-5, id sets equal
    beyond near-ties; queries whose probe set is ambiguous are left out."""
    c = _index(d)
    c.ix.nprobe = nprobe
    q = _queries(B, d, seed=B + k, x=c.x)
    D, I = c.ix.search(q, k)
    Do, Io, amb = np_sq_search(q, c.cent, c.codes, c.lists, *c.ranges, 0, nprobe, k)
    assert amb.mean() < 0.5
    _check(D, I, Do, Io, amb, f"d={d} nprobe={nprobe} k={k} B={B}")


@pytest.mark.parametrize("d", [256, 1024])
def test_batch_independence(d):
    """A query alone, in a batch of 33 and in a batch of 300: the same ids, D within 2e-6 (the bar of the IVF multi-block test); the
    same through the coalescer from 16 threads and through the device-buffer entry point."""
    import torch

    c = _index(d)
    c.ix.nprobe = 5
    q = _queries(300, d, 11, c.x)
    D300, I300 = c.ix.search(q, 40)
    D33, I33 = c.ix.search(q[:33], 40)
    assert np.array_equal(I33, I300[:33]) and np.abs(D33 - D300[:33]).max() <= 2e-6
    outs = [None] * 16

    def one(i):
        outs[i] = c.ix.search(q[i:i + 1], 40)

    th = [threading.Thread(target=one, args=(i,)) for i in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert np.array_equal(np.concatenate([o[1] for o in outs]), I300[:16])
    assert np.abs(np.concatenate([o[0] for o in outs]) - D300[:16]).max() <= 2e-6
    D1, I1 = c.ix.search(q[40:41], 40)  # alone, no other caller
    assert np.array_equal(I1[0], I300[40]) and np.abs(D1[0] - D300[40]).max() <= 2e-6
    qd = torch.from_numpy(q).cuda()
    Dd = torch.empty((300, 40), dtype=torch.float32, device="cuda")
    Id = torch.empty((300, 40), dtype=torch.int64, device="cuda")
    c.ix.search_device(qd.data_ptr(), 300, 40, Dd.data_ptr(), Id.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(Id.cpu().numpy(), I300) and np.abs(Dd.cpu().numpy() - D300).max() <= 2e-6


def test_padding_and_empty_lists():
    """Fewer rows than k in the probed lists -> -1 / -FLT_MAX padding; an empty probed list is walked without harm."""
    c = _index(768)
    c.ix.nprobe = 1
    empty, single = int(np.flatnonzero(SIZES == 0)[0]), int(np.flatnonzero(SIZES == 1)[0])
    q = np.ascontiguousarray(c.cent[[empty, single]].astype(np.float32))
    D, I = c.ix.search(q, 40)
    Do, Io, amb = np_sq_search(q, c.cent, c.codes, c.lists, *c.ranges, 0, 1, 40)
    assert not amb.any() and (Io[0] == -1).all() and (Io[1] >= 0).sum() == 1
    assert (I[0] == -1).all() and (D[0] == NEG).all()
    assert I[1, 0] == int(np.flatnonzero(c.lists == single)[0]) and (I[1, 1:] == -1).all() and (D[1, 1:] == NEG).all()
    _check(D, I, Do, Io, amb, "padding")
    c.ix.nprobe = 3  # the empty list together with two others, in a batch that mixes both kinds of query
    q2 = np.concatenate([q, _queries(31, 768, 5, c.x)])
    D, I = c.ix.search(q2, 64)
    Do, Io, amb = np_sq_search(q2, c.cent, c.codes, c.lists, *c.ranges, 0, 3, 64)
    _check(D, I, Do, Io, amb, "empty list among the probed")


# ------------------------------------------------------------------------------------------------ decoded rows
@pytest.mark.parametrize("d", [256, 1024])
def test_reconstruct_is_the_numpy_decode(d):
    """reconstruct_batch, the R of search_and_reconstruct and the rows behind search_dedup = vmin + (code + 0.5) * step bit for bit;
    id -1 -> 0xFF bytes; the dedup links are those of the decoded rows."""
    from clip_retrieval_amd.service import KnnHotPath, normalized

    c = _index(d)
    dec = np_sq_decode(c.codes, *c.ranges)
    ids = np.array([0, 17, N - 1, 1234, -1, 10], dtype=np.int64)
    R = c.ix.reconstruct_batch(ids)
    assert np.array_equal(R[4].view(np.uint32), np.full(d, 0xFFFFFFFF, np.uint32))
    ok = ids >= 0
    assert np.array_equal(R[ok].view(np.uint32), dec[ids[ok]].view(np.uint32))
    c.ix.nprobe = 1
    single = int(np.flatnonzero(SIZES == 1)[0])
    q = np.concatenate([_queries(5, d, 1, c.x), c.cent[[single]].astype(np.float32)])
    D, I, R = c.ix.search_and_reconstruct(q, 64)
    assert (I[5, 1:] == -1).all()
    want = np.where((I >= 0)[..., None], dec[np.maximum(I, 0)], np.full(d, -1, np.int32).view(np.float32)[None, None])
    assert np.array_equal(R.view(np.uint32), want.view(np.uint32))
    # dedup: the planted near-copies of row 10 sit in one list; query it
    c.ix.nprobe = NLIST
    qd = c.x[DUP[0]:DUP[0] + 1].astype(np.float32)
    D0, I0 = c.ix.search(qd, 40)
    D1, I1, R1, links = c.ix.search_dedup(qd, 40, 0.94, want_r=True)
    assert np.array_equal(I1, I0) and np.abs(D1 - D0).max() <= 2e-6
    assert np.array_equal(R1[0].view(np.uint32), dec[I1[0]].view(np.uint32))
    assert set(DUP) <= set(I1[0].tolist())
    Rn = normalized(dec[I1[0]])
    s = Rn @ Rn.T
    want_links = [(i, j) for i in range(40) for j in range(i + 1, 40) if s[i, j] > 0.94]
    near = {(i, j) for i in range(40) for j in range(i + 1, 40) if abs(s[i, j] - 0.94) < 1e-5}
    got = [tuple(int(v) for v in p) for p in links]
    assert len(got) >= 6 and set(got) - near == set(want_links) - near and got == sorted(got)
    if not near:
        assert KnnHotPath.non_uniques_from_pairs(links, 40) == KnnHotPath.non_uniques_from_pairs(np.asarray(want_links, dtype=np.int32).reshape(-1, 2), 40)


def test_ranking_is_practically_ivf_flats():
    """Same centroids, nprobe = nlist, mixture corpus at d = 256: mean top-10 overlap with IVF-Flat >= 0.95 -- the CPU condition, now
    through the kernels."""
    from clip_retrieval_amd.knn import build_ivf_index, build_ivfsq_index, train_ivf_centroids

    n, d, nlist = 6000, 256, 24
    x = synth_mixture_rows(np.arange(n), d, 7, MIX_CLUSTERS)
    cent = train_ivf_centroids(x, nlist, niter=3, seed=0)
    flat = build_ivf_index(x, nlist, nprobe=nlist, centroids=cent)
    sq = build_ivfsq_index(x, nlist, nprobe=nlist, centroids=cent)  # ranges trained on the rows
    assert np.array_equal(np.stack(sq.sq_quantizer()), np.stack(np_ranges(x)))
    q = _queries(64, d, 4, x)
    Df, If = flat.search(q, 10)
    Ds, Is = sq.search(q, 10)
    ov = float(np.mean([len(set(a) & set(b)) / 10 for a, b in zip(If.tolist(), Is.tolist())]))
    print(f"top-10 overlap with IVF-Flat: {ov:.4f}; max |D_sq - D_flat| on shared ids: "
          f"{max(abs(Ds[i][list(Is[i]).index(j)] - Df[i][list(If[i]).index(j)]) for i in range(64) for j in set(If[i]) & set(Is[i])):.2e}")
    assert ov >= 0.95
    exact = q.astype(np.float64) @ x.astype(np.float64).T
    assert top10_overlap(exact, exact) == 1.0
    flat.close()
    sq.close()


# ------------------------------------------------------------------------------------------------ the other paths
def test_two_shards_and_a_mixed_adopt():
    from clip_retrieval_amd import HipLibraryError, knn

    c = _index(768)
    cut = [0, 1300, N]
    mk = lambda g, ranges: knn._ivfsq_encode_chunks(iter([(0, c.x[cut[g]:cut[g + 1]])]), cut[g + 1] - cut[g], 768, NLIST, c.cent, ranges,  # pylint: disable=protected-access
                                                    c.lists[cut[g]:cut[g + 1]], 5, 0, cut[g])
    shards = [mk(0, c.ranges), mk(1, c.ranges)]
    sh = knn.ShardedMi355xIndex.from_shards(shards, cut[:2])
    sh.nprobe = 5
    c.ix.nprobe = 5
    q = _queries(40, 768, 4, c.x)
    D, I = sh.search(q, 40)
    D0, I0 = c.ix.search(q, 40)
    assert np.array_equal(I, I0) and np.abs(D - D0).max() <= 2e-6
    dec = np_sq_decode(c.codes, *c.ranges)
    assert np.array_equal(sh.reconstruct_batch(I[0]).view(np.uint32), dec[I[0]].view(np.uint32))
    sh.close()
    other = (c.ranges[0], (c.ranges[1] * np.float32(1.5)).astype(np.float32))
    a, b = mk(0, c.ranges), mk(1, other)
    with pytest.raises(HipLibraryError, match="IVF-SQ8 shards carry different quantisers"):
        knn.ShardedMi355xIndex.from_shards([a, b], cut[:2])
    a.close()
    b.close()


def test_save_load_round_trip(tmp_path):
    """Built from a folder of embeddings, saved, embeddings deleted, loaded through add_codes: identical D and I; as two shards too."""
    import shutil

    from clip_retrieval_amd import knn

    n, d, nlist = 5000, 512, 32
    rng = np.random.default_rng(31)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)
    emb = tmp_path / "emb"
    emb.mkdir()
    np.save(emb / "img_emb_0.npy", x[:3000])
    np.save(emb / "img_emb_1.npy", x[3000:])
    built = knn.build_ivfsq_index_from_folder(str(emb), **knn.ivfsq_params_from_index_key("IVF32,SQ8"), nprobe=8, niter=3, chunk=2048)
    assert built.is_sq and built.nlist == nlist
    q = _queries(40, d, 5, x)
    D0, I0 = built.search(q, 40)
    out = str(tmp_path / "idx")
    man = knn.save_index(built, out)
    assert man["kind"] == "ivfsq"
    built.close()
    shutil.rmtree(emb)
    assert sorted(os.listdir(out)) == sorted(["ivf_sq_centroids.npy", "ivf_sq_vmin.npy", "ivf_sq_vdiff.npy", "ivf_sq_codes.npy",
                                              "ivf_sq_lists.npy", knn.IVFSQ_MANIFEST])
    loaded = knn.load_index(out)
    assert loaded.is_sq and loaded.nprobe == 8 and loaded.ntotal == n
    D1, I1 = loaded.search(q, 40)
    assert np.array_equal(I0, I1) and np.array_equal(D0.view(np.uint32), D1.view(np.uint32))
    loaded.close()
    part = knn.load_index(out, row_range=(1000, 4000))
    assert part.ntotal == 3000 and part.search(q[:1], 5)[1].min() >= 1000
    part.close()
    sharded = knn.load_index(out, devices=[0, 0])
    D2, I2 = sharded.search(q, 40)
    assert np.array_equal(I0, I2) and np.abs(D0 - D2).max() <= 2e-6
    sharded.close()


def test_list_ordered_ids_and_the_hot_path():
    """ivf_old_to_new = the numpy restatement of the layout; KnnHotPath.knn_search serves k = 40 with the dedup on."""
    from clip_retrieval_amd.service import KnnHotPath

    c = _index(768)
    o2n = c.ix.ivf_old_to_new()
    assert np.array_equal(o2n, np_layout_old_to_new(c.lists, NLIST))
    n2o = c.ix.ivf_new_to_old()
    assert np.array_equal(n2o[o2n], np.arange(N))
    assert np.array_equal(c.ix.map_ids(np.array([5, -1, N - 1])), np.array([o2n[5], -1, o2n[N - 1]]))
    c.ix.nprobe = 5
    q = _queries(3, 768, 9, c.x)
    D, I = c.ix.search(q, 40)
    hot, res = KnnHotPath(), SimpleNamespace(image_index=c.ix, text_index=c.ix)
    for i in range(3):
        Dh, Ih = hot.knn_search(q[i:i + 1], "image", 40, res, False, False, False)
        keep = I[i] >= 0
        assert np.array_equal(np.asarray(Ih), I[i][keep]) and np.abs(np.asarray(Dh, dtype=np.float32) - D[i][keep]).max() <= 2e-6
        _, Ih = hot.knn_search(q[i:i + 1], "image", 40, res, True, False, False)
        assert set(Ih) <= set(I[i].tolist()) and len(Ih) >= 1


def test_refusals():
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import Mi355xIndex

    c = _index(256)
    q = _queries(2, 256, 1, c.x)
    with pytest.raises(HipLibraryError, match=r"code -5\): k > 64 is not supported on an IVF-SQ8 index"):
        c.ix.search(q, 65)
    with pytest.raises(HipLibraryError, match=r"code -5\): range_search is not supported on an IVF-SQ8 index"):
        c.ix.range_search(q, 0.5)
    for call in (lambda: c.ix.add(c.x[:3]), c.ix.reset, lambda: c.ix.reserve(10), lambda: c.ix.synth_fill(10, 1),
                 lambda: c.ix.set_sq_quantizer(*c.ranges)):
        with pytest.raises(HipLibraryError, match=r"code -4\).*IVF-SQ8"):
            call()
    pq = Mi355xIndex(256)
    pq.set_pq_quantizer(16, np.zeros(256 * 256, np.float32))
    with pytest.raises(HipLibraryError, match=r"code -4\).*IVF-SQ8"):
        pq.set_sq_quantizer(*c.ranges)
    pq.close()
    flat = Mi355xIndex(256)
    flat.add(c.x[:10])
    with pytest.raises(HipLibraryError, match=r"code -4\).*IVF-SQ8"):
        flat.set_sq_quantizer(*c.ranges)
    assert not flat.is_sq
    flat.close()
    e = Mi355xIndex(256)
    bad = c.ranges[1].copy()
    bad[3] = -1
    with pytest.raises(HipLibraryError, match=r"code -1\).*IVF-SQ8"):
        e.set_sq_quantizer(c.ranges[0], bad)
    bad[3] = np.inf
    with pytest.raises(HipLibraryError, match=r"code -1\).*IVF-SQ8"):
        e.set_sq_quantizer(c.ranges[0], bad)
    e.set_sq_quantizer(*c.ranges)
    with pytest.raises(HipLibraryError, match=r"code -4\).*IVF-SQ8"):
        e.set_pq_quantizer(16, np.zeros(256 * 256, np.float32))
    e.close()


def test_ivf_flat_next_to_it_is_unchanged():
    """An IVF-Flat index built before and after an IVF-SQ8 one in the same process returns identical D, I."""
    from clip_retrieval_amd.knn import build_ivf_index, build_ivfsq_index

    c = _index(768)
    q = _queries(70, 768, 2, c.x)

    def flat_answer():
        ix = build_ivf_index(c.x, NLIST, nprobe=5, centroids=c.cent)
        out = ix.search(q, 40), ix.search(q[:1], 40), ix.reconstruct_batch(np.arange(5))
        assert not ix.is_sq
        ix.close()
        return out

    before = flat_answer()
    sq = build_ivfsq_index(c.x, NLIST, nprobe=5, centroids=c.cent, ranges=c.ranges)
    sq.search(q, 40)
    sq.close()
    after = flat_answer()
    for a, b in zip(before, after):
        if isinstance(a, tuple):
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        else:
            assert np.array_equal(a, b)
