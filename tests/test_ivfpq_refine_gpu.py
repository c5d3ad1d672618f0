"""The refine store of IVF-PQ (faiss IndexRefineFlat(IndexIVFPQ), with or without the OPQ rotation) on the GPU against the numpy
restatement of test_ivfpq_refine_cpu.py, built from the index's own codes: search parity, long lists, exact ties, the rotation, the
stored rows, the other entry points, the build forms and the state rules, recall."""
import shutil
import threading

import numpy as np
import pytest

from oracle.knn_oracle import synth_mixture_rows, topk_sets_equal
from test_ivfpq_gpu import CASES, _data, _queries, _seed_codebooks
from test_ivfpq_refine_cpu import TOL, check_refine, np_refine_parts, np_refine_search
from test_opq_cpu import random_rotation

pytestmark = pytest.mark.gpu


def _lists_of(y, cent):
    from clip_retrieval_amd.knn import IvfBuilder

    b = IvfBuilder(y.shape[1], cent.shape[0])
    b.set_centroids(cent)
    lists = b.assign(y)
    b.close()
    return lists


def _small_index(n, d, nlist, M, nprobe, seed, refine=True, k_factor=1, x=None, id_base=0):
    """_small_index of test_ivfpq_gpu.py (same seeds, same centroids, lists and codebooks) with a refine store."""
    from clip_retrieval_amd.knn import build_ivfpq_index

    x = _data(n, d, seed) if x is None else x
    cent = x[np.random.default_rng(seed + 1).choice(n, nlist, replace=False)]
    lists = _lists_of(x, cent)
    cb = _seed_codebooks(x, cent, lists, M, seed + 2)
    ix = build_ivfpq_index(x, nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb, refine=refine, k_factor=k_factor, id_base=id_base)
    return x, cent, cb, ix


def _rotated_index(n, d, nlist, M, nprobe, seed, k_factor=1):
    """_rotated_index of test_opq_gpu.py with a refine store -> x, A, cent, cb, index (cent, cb in the rotated space)."""
    from clip_retrieval_amd.knn import build_ivfpq_index, rotate_rows

    x = _data(n, d, seed)
    A = random_rotation(d, seed + 7)
    y = rotate_rows(A, x)
    cent = y[np.random.default_rng(seed + 1).choice(n, nlist, replace=False)]
    cb = _seed_codebooks(y, cent, _lists_of(y, cent), M, seed + 2)
    ix = build_ivfpq_index(x, nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb, rotation=A, refine=True, k_factor=k_factor)
    return x, A, cent, cb, ix


def _parity(ix, x, cent, cb, q, nprobe, k, kf, ctx, qc=None, id_base=0):
    codes, lists = ix.pq_codes()
    parts, amb = np_refine_parts(q, x, cent, cb, codes, lists, id_base, nprobe, qc=qc)
    assert amb.mean() < 0.5
    D, I = ix.search(q, k)
    worst = check_refine(D, I, parts, amb, k, k * kf, ctx)
    print(f"{ctx}: max |D - E| = {worst:.2e}, ambiguous probe sets {amb.mean():.2f}")
    return D, I, parts, amb


# ------------------------------------------------------------------------------------------------ 1. parity
# CASES of test_ivfpq_gpu.py x k_factor: every d, every M, B in {1, 31, 33, 256, 300}; kc = 512 at M = 128 (the LDS worst case, once with
# far fewer probed rows than kc and once selected from ~4 000) and at M = 16; nprobe 1 with kc = 512 (a list holds ~52 rows: the result
# is the exact top k of the list, padded at k = 64); kc <= 64 (the plain scan's queues) and kc > 64 (the workgroup queue)
KF = [8, 8, 8, 1, 8, 12, 8, 64, 2, 8]
REFINE_CASES = [c + (kf,) for c, kf in zip(CASES, KF)] + [(1024, 128, 80, 1, 64, 8)]


@pytest.mark.parametrize("d,M,nprobe,B,k,kf", REFINE_CASES)
def test_search_parity(d, M, nprobe, B, k, kf):
    n, nlist = 5000, 96
    nprobe = nlist if nprobe == "nlist" else nprobe
    x, cent, cb, ix = _small_index(n, d, nlist, M, nprobe, seed=d + M, k_factor=kf)
    assert ix.pq_refine and ix.k_factor == kf and ix.pq_m == M and ix.ntotal == n
    q = _queries(B, d, seed=B + k, x=x)
    D, I, parts, amb = _parity(ix, x, cent, cb, q, nprobe, k, kf, f"d={d} M={M} nprobe={nprobe} B={B} k={k} k_factor={kf}")
    if nprobe == 1:  # kc far above a list's rows: the exact top k of the probed list
        Ds, Is = np_refine_search(parts, k, k * kf)
        ok = ~amb
        assert np.array_equal(I[ok] >= 0, Is[ok] >= 0)
        assert not topk_sets_equal(I[ok], D[ok], Is[ok], Ds[ok].astype(np.float32), tol=TOL)
    ix.close()


def test_k_factor_1_returns_the_plain_ids_and_513_is_refused():
    from clip_retrieval_amd import HipLibraryError
    from test_ivfpq_gpu import _small_index as plain_index

    d, M, nprobe, B, k = CASES[3]
    x, cent, cb, plain = plain_index(5000, d, 96, M, 96, seed=d + M)
    _, _, _, ix = _small_index(5000, d, 96, M, 96, seed=d + M)
    assert ix.k_factor == 1 and not plain.pq_refine
    assert np.array_equal(ix.pq_codes()[0], plain.pq_codes()[0])
    q = _queries(B, d, seed=B + k, x=x)
    Dp, Ip = plain.search(q, k)
    D, I = ix.search(q, k)
    # the same ids (ADC near-ties at the k-th place aside), ranked by their exact scores
    parts, _ = np_refine_parts(q, x, cent, cb, *ix.pq_codes(), 0, 96)
    S = np.array([p[1][np.searchsorted(p[0], row)] for p, row in zip(parts, I)], dtype=np.float32)  # (p[0]: ascending ids)
    order = np.argsort(-S, axis=1, kind="stable")
    assert not topk_sets_equal(np.take_along_axis(I, order, 1), np.take_along_axis(S, order, 1), Ip, Dp, tol=TOL)
    assert (np.diff(D, axis=1) <= 0).all()
    # k x k_factor beyond 512: refused with both numbers
    ix.k_factor = 27
    with pytest.raises(HipLibraryError, match=r"19 x 27"):
        ix.search(q[:3], 19)
    ix.k_factor = 8
    assert ix.search(q[:3], 64)[1].shape == (3, 64)
    plain.close()
    ix.close()


# ------------------------------------------------------------------------------------------------ 2. long lists
def test_long_lists_prune_and_batch_independence():
    """~2 500 rows per list, kc = 512: every workgroup sees several times kc rows, so its queue is pruned; B = 300 is two passes with
    another share count than B = 1.  A query's I and the bits of its D do not depend on the batch it travels in."""
    n, d, nlist, M, nprobe, k, kf = 20000, 512, 8, 16, 8, 64, 8
    x, cent, cb, ix = _small_index(n, d, nlist, M, nprobe, seed=77, k_factor=kf)
    q = _queries(300, d, seed=5, x=x)
    codes, lists = ix.pq_codes()
    parts, amb = np_refine_parts(q, x, cent, cb, codes, lists, 0, nprobe)
    res = {}
    for B in (1, 33, 300):
        D, I = ix.search(q[:B], k)
        worst = check_refine(D, I, parts[:B], amb[:B], k, k * kf, f"long lists B={B}")
        print(f"long lists B={B}: max |D - E| = {worst:.2e}")
        res[B] = (D, I)
    for B in (1, 33):
        assert np.array_equal(res[B][1], res[300][1][:B]), f"B={B}: ids depend on the batch"
        assert np.array_equal(res[B][0].view(np.uint32), res[300][0][:B].view(np.uint32)), f"B={B}: score bits depend on the batch"
    for i in (0, 7, 32, 299):
        D1, I1 = ix.search(q[i:i + 1], k)
        assert np.array_equal(I1[0], res[300][1][i]) and np.array_equal(D1[0].view(np.uint32), res[300][0][i].view(np.uint32)), i
    ix.close()


# ------------------------------------------------------------------------------------------------ 3. exact ties
def test_exact_ties_go_to_the_lowest_ids():
    """600 byte-identical copies of one row at scattered ids: identical codes, identical fp32 ADC sums, identical exact scores.  The
    candidates are the 160 lowest ids of the copies and the result is the 40 lowest."""
    n, d, nlist, M, k, kf = 5000, 512, 16, 32, 40, 4
    x = _data(n, d, 13)
    cent_rows = np.random.default_rng(13 + 1).choice(n, nlist, replace=False)  # (_small_index's draw: no copy becomes a centroid)
    where = np.sort(np.random.default_rng(14).choice(np.setdiff1d(np.arange(n), cent_rows), 600, replace=False))
    x[where] = x[where[0]]
    _, cent, cb, ix = _small_index(n, d, nlist, M, 4, seed=13, k_factor=kf, x=x)
    codes, lists = ix.pq_codes()
    assert len(set(lists[where].tolist())) == 1 and (codes[where] == codes[where[0]]).all()
    q = x[where[:1]].astype(np.float32)
    D, I = ix.search(q, k)
    assert np.array_equal(I[0], where[:k]), "exact ties: not the lowest ids"
    assert (D[0] == D[0, 0]).all()
    # the candidate stage alone: with k_factor 1 a result is the candidate set
    ix.k_factor = 1
    _, Ic = ix.search(q, 64)
    assert np.array_equal(Ic[0], where[:64])
    ix.k_factor = 8  # kc = 512 through the workgroup queue: 512 of the 600 tie, the 64 lowest come back
    _, Ic = ix.search(q, 64)
    assert np.array_equal(Ic[0], where[:64])
    ix.close()


# ------------------------------------------------------------------------------------------------ 4. rotation
def test_search_parity_rotated():
    """Behind an OPQ rotation: candidates from the rotated-space restatement, scores within 1e-5 of q . x in the ORIGINAL space."""
    d, M, nprobe, B, k = CASES[0]
    kf = 8
    x, A, cent, cb, ix = _rotated_index(5000, d, 96, M, nprobe, seed=d + M, k_factor=kf)
    assert ix.pq_refine and np.array_equal(ix.pq_rotation(), A)
    q = _queries(B, d, seed=B + k, x=x)
    qc = (q.astype(np.float64) @ A.astype(np.float64).T).astype(np.float32)
    _parity(ix, x, cent, cb, q, nprobe, k, kf, f"rotated d={d} M={M} k_factor={kf}", qc=qc)
    ids = np.array([3, 4999, -1, 17], dtype=np.int64)
    R = ix.reconstruct_batch(ids)
    assert np.array_equal(R[[0, 1, 3]].view(np.uint32), x[[3, 4999, 17]].astype(np.float32).view(np.uint32)), "no back-rotation of stored rows"
    ix.close()


# ------------------------------------------------------------------------------------------------ 5. rows
def test_rows_are_the_stored_rows():
    n, d = 4000, 768
    x = _data(n, d, 23)
    # planted near-duplicates: pairs closer than 0.94 whose DECODED vectors (1 byte per 12 dimensions) would not link
    rng = np.random.default_rng(24)
    base = rng.choice(n // 2, 40, replace=False)
    x[base + n // 2] = (x[base].astype(np.float32) + 0.2 * rng.standard_normal((40, d)).astype(np.float32) / np.sqrt(d)).astype(np.float16)
    _, cent, cb, ix = _small_index(n, d, 16, 64, 16, seed=23, k_factor=4, x=x)
    q = x[base[:6]].astype(np.float32)
    D, I, R = ix.search_and_reconstruct(q, 40)
    want = x[np.maximum(I, 0)].astype(np.float32)
    want.view(np.uint32)[I < 0] = 0xFFFFFFFF
    assert np.array_equal(R.view(np.uint32), want.view(np.uint32)), "R is not f32(x[I]) bit for bit"
    ids = np.array([0, 17, n - 1, 1234, -1, n], dtype=np.int64)
    Rb = ix.reconstruct_batch(ids)
    assert np.array_equal(Rb[:4].view(np.uint32), x[ids[:4]].astype(np.float32).view(np.uint32))
    assert (Rb[4:].view(np.uint32) == 0xFFFFFFFF).all()
    linked = 0
    for i in range(len(q)):
        D1, I1, R1, pairs = ix.search_dedup(q[i:i + 1], 40, threshold=0.94, want_r=True)
        assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0].view(np.uint32), D[i].view(np.uint32))
        assert np.array_equal(R1[0].view(np.uint32), R[i].view(np.uint32))
        v = x[I[i]].astype(np.float64)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        g = v @ v.T
        clear = np.abs(g - 0.94) > 1e-5  # (pairs within fp32 rounding of the threshold may go either way)
        got = np.zeros_like(clear)
        got[pairs[:, 0], pairs[:, 1]] = True
        iu = np.triu(np.ones_like(clear), 1)
        assert np.array_equal((got & clear)[iu], ((g > 0.94) & clear)[iu]), f"query {i}: dedup links differ from those of the exact rows"
        linked += int(got.sum())
    assert linked >= len(q), "the planted duplicates were not linked"
    ix.close()


# ------------------------------------------------------------------------------------------------ 6. entry points
def test_entry_points():
    import torch

    from clip_retrieval_amd.service import KnnHotPath

    x, cent, cb, ix = _small_index(4000, 512, 32, 32, 8, seed=9, k_factor=8)
    q = _queries(48, 512, 2, x)
    D, I = ix.search(q, 40)
    qd = torch.from_numpy(q).cuda()
    Dd = torch.empty((len(q), 40), dtype=torch.float32, device="cuda")
    Id = torch.empty((len(q), 40), dtype=torch.int64, device="cuda")
    ix.search_device(qd.data_ptr(), len(q), 40, Dd.data_ptr(), Id.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(Id.cpu().numpy(), I) and np.array_equal(Dd.cpu().numpy().view(np.uint32), D.view(np.uint32))
    outs = [None] * 16

    def one(i):
        outs[i] = ix.search(q[i:i + 1], 40)

    th = [threading.Thread(target=one, args=(i,)) for i in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert np.array_equal(np.concatenate([o[1] for o in outs]), I[:16])
    assert np.array_equal(np.concatenate([o[0] for o in outs]).view(np.uint32), D[:16].view(np.uint32))
    from types import SimpleNamespace

    hot, res = KnnHotPath(), SimpleNamespace(image_index=ix, text_index=ix)
    for i in range(3):  # no code of its own for a refine index: without and with the fused dedup
        Dh, Ih = hot.knn_search(q[i:i + 1], "image", 40, res, False, False, False)
        assert np.array_equal(np.asarray(Ih), I[i]) and np.array_equal(np.asarray(Dh, dtype=np.float32), D[i])
        _, Ih = hot.knn_search(q[i:i + 1], "image", 40, res, True, False, False)
        assert set(Ih) <= set(I[i].tolist()) and len(Ih) >= 1
    ix.close()


def test_two_refine_shards_and_a_mixed_adopt():
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import ShardedMi355xIndex, build_ivfpq_index

    n, d, nlist, M, nprobe, k, kf = 6000, 768, 48, 32, 6, 40, 4
    x = _data(n, d, 21)
    cent = x[np.random.default_rng(2).choice(n, nlist, replace=False)]
    lists = _lists_of(x, cent)
    cb = _seed_codebooks(x, cent, lists, M, 3)
    cut = [0, 2500, n]

    def shard(g, refine):
        return build_ivfpq_index(x[cut[g]:cut[g + 1]], nlist, M, nprobe=nprobe, id_base=cut[g], centroids=cent, codebooks=cb, refine=refine,
                                 k_factor=kf)

    shards = [shard(0, True), shard(1, True)]
    codes = [s.pq_codes()[0] for s in shards]
    q = _queries(20, d, 4, x)
    # every shard refines its own kc candidates; the merge ranks the exact scores
    per = []
    amb = None
    for g in range(2):
        parts, amb = np_refine_parts(q, x[cut[g]:cut[g + 1]], cent, cb, codes[g], lists[cut[g]:cut[g + 1]], cut[g], nprobe)
        per.append(parts)
    ix = ShardedMi355xIndex.from_shards(shards, cut[:2])
    assert ix.pq_refine and ix.k_factor == kf
    D, I = ix.search(q, k)
    Ds = [np_refine_search(p, k, k * kf) for p in per]
    Dm = np.concatenate([Ds[0][0], Ds[1][0]], axis=1)
    Im = np.concatenate([Ds[0][1], Ds[1][1]], axis=1)
    order = np.lexsort((Im, -Dm), axis=1)[:, :k]
    Do, Io = np.take_along_axis(Dm, order, 1), np.take_along_axis(Im, order, 1)
    ok = ~amb
    assert np.abs(D[ok].astype(np.float64) - Do[ok]).max() <= TOL
    assert not topk_sets_equal(I[ok], D[ok], Io[ok], Do[ok].astype(np.float32), tol=TOL)
    ix.k_factor = 2
    assert ix.k_factor == 2
    ix.close()
    mixed = [shard(0, True), shard(1, False)]
    with pytest.raises(HipLibraryError, match="with and without a refine store"):
        ShardedMi355xIndex.from_shards(mixed, cut[:2])
    for s in mixed:
        s.close()


# ------------------------------------------------------------------------------------------------ 7. build forms and state
def test_device_build_equals_host_build():
    import ctypes as C

    import torch

    from clip_retrieval_amd.knn import build_ivfpq_index_device

    n, d, nlist, M = 7000, 768, 24, 64
    x, cent, cb, host = _small_index(n, d, nlist, M, 4, seed=41, k_factor=4)
    xd = torch.from_numpy(x).cuda()
    handed = []

    def fill_rows(dst, row0, count, stride):  # device rows -> dst, completed on return
        handed.append((row0, count, stride))
        src = xd[row0:row0 + count * stride:stride][:count].contiguous()
        torch.cuda.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src.data_ptr()), src.numel() * 2, 3) == 0  # device to device
        torch.cuda.synchronize()  # (a device-to-device hipMemcpy does not wait on the host: without this the copy is not "completed on return")

    dev, stats = build_ivfpq_index_device(fill_rows, n, d, nlist, M, nprobe=4, centroids=cent, codebooks=cb, chunk=3000, refine=True, k_factor=4)
    c0, l0 = host.pq_codes()
    c1, l1 = dev.pq_codes()
    assert np.array_equal(l0, l1) and np.array_equal(c0, c1)
    ids = np.arange(n, dtype=np.int64)
    assert np.array_equal(dev.reconstruct_batch(ids).view(np.uint32), x.astype(np.float32).view(np.uint32))
    assert np.array_equal(host.reconstruct_batch(ids).view(np.uint32), x.astype(np.float32).view(np.uint32))
    assert dev.pq_refine and dev.k_factor == 4
    assert len(handed) == 2 * 3, "one assignment and one encoding pass over the three chunks, nothing generated a third time"
    assert stats["bytes_per_row"] == M + 12 + 2 * d
    tiles = sum((s + 31) // 32 for s in np.bincount(l0, minlength=nlist))
    assert stats["row_arena_bytes"] == tiles * 32 * d * 2 and stats["code_arena_bytes"] == tiles * 32 * M
    q = _queries(9, d, 3, x)
    Dh, Ih = host.search(q, 40)
    Dd, Id = dev.search(q, 40)
    assert np.array_equal(Ih, Id) and np.array_equal(Dh.view(np.uint32), Dd.view(np.uint32))
    host.close()
    dev.close()


def test_save_and_load_need_the_embeddings(tmp_path):
    from clip_retrieval_amd import knn

    n, d, nlist, M = 5000, 512, 32, 64
    emb = tmp_path / "emb"
    emb.mkdir()
    x = _data(n, d, 31)
    np.save(emb / "img_emb_0.npy", x[:3000])
    np.save(emb / "img_emb_1.npy", x[3000:])
    A = random_rotation(d, 5)
    built = knn.build_ivfpq_index_from_folder(str(emb), nlist, M, nprobe=8, niter=3, pq_niter=3, chunk=2048, rotation=A, refine=True, k_factor=4)
    q = _queries(40, d, 5, x)
    D0, I0 = built.search(q, 40)
    out = str(tmp_path / "idx")
    man = knn.save_index(built, out)
    built.close()
    assert man["refine"] is True and man["k_factor"] == 4
    loaded = knn.load_index(out)
    assert loaded.pq_refine and loaded.k_factor == 4 and loaded.pq_m == M and loaded.nprobe == 8
    D1, I1 = loaded.search(q, 40)
    assert np.array_equal(I0, I1) and np.array_equal(D0.view(np.uint32), D1.view(np.uint32))
    assert np.array_equal(loaded.reconstruct_batch(np.arange(n)).view(np.uint32), x.astype(np.float32).view(np.uint32))
    loaded.close()
    sharded = knn.load_index(out, devices=[0, 0])
    D2, I2 = sharded.search(q, 10)
    assert sharded.pq_refine and (np.diff(D2, axis=1) <= 0).all() and (I2 >= 0).all()
    sharded.close()
    # a corrupted code file: the rows no longer encode to it
    codes = np.load(tmp_path / "idx" / "ivf_pq_codes.npy")
    good = codes.copy()
    codes[17, 3] ^= 1
    np.save(tmp_path / "idx" / "ivf_pq_codes.npy", codes)
    with pytest.raises(ValueError, match="do not encode to the saved ivf_pq_codes.npy"):
        knn.load_index(out)
    np.save(tmp_path / "idx" / "ivf_pq_codes.npy", good)
    # the embeddings gone: refused with a clear message; named elsewhere: found
    moved = tmp_path / "elsewhere"
    shutil.move(str(emb), str(moved))
    with pytest.raises(FileNotFoundError, match="needs the embeddings"):
        knn.load_index(out)
    again = knn.load_index(out, embeddings_folder=str(moved))
    D3, I3 = again.search(q, 40)
    assert np.array_equal(I0, I3) and np.array_equal(D0.view(np.uint32), D3.view(np.uint32))
    again.close()


def test_state_rules():
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import Mi355xIndex, build_ivf_index

    x, cent, cb, ix = _small_index(1000, 512, 8, 16, 2, seed=1, k_factor=2)
    q = _queries(2, 512, 1, x)
    with pytest.raises(HipLibraryError, match="after knnx_ivfpq_set_quantizer and before knnx_ivf_begin"):
        ix.set_pq_refine()  # a built index
    for bad in (0, 513):
        with pytest.raises(HipLibraryError, match=r"k_factor must lie in 1 \.\. 512"):
            ix.k_factor = bad
    assert ix.k_factor == 2
    with pytest.raises(HipLibraryError, match="k > 64 is not supported on an IVF-PQ index"):
        ix.search(q, 65)
    with pytest.raises(HipLibraryError, match="range_search is not supported on an IVF-PQ index"):
        ix.range_search(q, 0.5)
    ix.close()
    flat = Mi355xIndex(512)
    with pytest.raises(HipLibraryError, match="after knnx_ivfpq_set_quantizer"):
        flat.set_pq_refine()
    flat.close()
    ivf = build_ivf_index(x, 8, nprobe=2, niter=2)
    with pytest.raises(HipLibraryError, match="after knnx_ivfpq_set_quantizer"):
        ivf.set_pq_refine()
    ivf.close()
    # between begin and end: the choice is closed, and precomputed codes have no rows to store
    b = Mi355xIndex(512)
    b.set_pq_quantizer(16, cb)
    b.set_pq_refine()
    assert b.pq_refine
    sizes = np.array([2, 1] + [0] * 6, dtype=np.int64)
    lib, h = b._lib, b._h  # pylint: disable=protected-access
    assert lib.knnx_ivf_begin(h, 8, np.ascontiguousarray(cent).ctypes.data, sizes.ctypes.data) == 0
    with pytest.raises(HipLibraryError, match="before knnx_ivf_begin"):
        b.set_pq_refine(False)
    codes = np.zeros((3, 16), np.uint8)
    ids, ls, pos = np.arange(3, dtype=np.int64), np.array([0, 0, 1], np.int32), np.array([0, 1, 0], np.int32)
    rc = lib.knnx_ivfpq_add_codes(h, codes.ctypes.data, 3, ids.ctypes.data, ls.ctypes.data, pos.ctypes.data)
    assert rc != 0 and b"no rows to store" in lib.knnx_last_error()
    b.close()
    # a plain IVF-PQ index of the same process refuses nothing new and decodes as before
    from test_ivfpq_gpu import _small_index as plain_index

    xp, centp, cbp, plain = plain_index(1000, 512, 8, 16, 2, seed=1)
    assert not plain.pq_refine and plain.k_factor == 1
    plain.k_factor = 8  # no effect without a refine store
    codes, lists = plain.pq_codes()
    R = plain.reconstruct_batch(np.array([5], dtype=np.int64))
    assert np.array_equal(R[0], centp[lists[5]].astype(np.float32) + cbp[np.arange(16), codes[5]].reshape(-1))
    assert plain.pq_arena_bytes()[1] == 0
    Dk, Ik = plain.search(q, 10)
    plain.k_factor = 1
    D1, I1 = plain.search(q, 10)
    assert np.array_equal(Ik, I1) and np.array_equal(Dk, D1)
    plain.close()


# ------------------------------------------------------------------------------------------------ 8. quality
def test_refine_recall():
    """Recall@10 against the exact flat top-10: at least the numpy restatement's on the index's own codes minus 0.02 (the boundary
    band), strictly above the plain index's, at most 1."""
    from clip_retrieval_amd.knn import PqBuilder, build_ivfpq_index, train_ivf_centroids, train_pq_codebooks

    n, d, nlist, M, nc, k, kf = 6000, 512, 16, 32, 40, 10, 8
    x = synth_mixture_rows(np.arange(n), d, 7, nc)
    cent = train_ivf_centroids(x, nlist, niter=4, seed=0)
    lists = _lists_of(x, cent)
    pb = PqBuilder(d, M)
    pb.set_sample(x, lists, cent)
    cb = train_pq_codebooks(pb, niter=6, seed=3)
    pb.close()
    q = _queries(64, d, 8, x)
    exact = np.argsort(-(q @ x.astype(np.float32).T), axis=1)[:, :k]

    def recall(I):
        return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(I, exact)]))

    plain = build_ivfpq_index(x, nlist, M, nprobe=nlist, centroids=cent, codebooks=cb)
    r_plain = recall(plain.search(q, k)[1])
    plain.close()
    ix = build_ivfpq_index(x, nlist, M, nprobe=nlist, centroids=cent, codebooks=cb, refine=True, k_factor=kf)
    r_dev = recall(ix.search(q, k)[1])
    parts, _ = np_refine_parts(q, x, cent, cb, *ix.pq_codes(), 0, nlist)
    r_np = recall(np_refine_search(parts, k, k * kf)[1])
    ix.close()
    print(f"recall@10: plain IVF-PQ {r_plain:.3f}, refine k_factor {kf} {r_dev:.3f}, numpy restatement {r_np:.3f}")
    assert r_dev >= r_np - 0.02, (r_dev, r_np)
    assert r_plain < r_dev <= 1.0, (r_plain, r_dev)
