"""OPQ rotation in front of IVF-PQ (faiss IndexPreTransform(OPQMatrix(d, M), IndexIVFPQ(...)), d_out = d_in): the row-rotation kernel,
search parity with the numpy restatement of tests/test_ivfpq_gpu.py in the rotated space, a permutation as the rotation,
reconstruction in the original space, the other entry points, refusals and training."""
import json
import os
import threading

import numpy as np
import pytest

from test_ivfpq_gpu import CASES, _check, _data, _queries, _seed_codebooks, codes_match, np_adc_search, np_encode
from test_opq_cpu import BAND, CAP, ROT_CASES, heavy_rows, np_opq, random_rotation, rotation_band, unit_rows

pytestmark = pytest.mark.gpu


def _rotated_index(n, d, nlist, M, nprobe, seed, A=None, id_base=0, x=None):
    """_small_index of test_ivfpq_gpu.py behind a rotation: random rows as centroids, codebooks from residual sub-vectors of random
    rows -- all in the rotated space, y = the device's own rotated rows.  -> x, y, A, cent, cb, index"""
    from clip_retrieval_amd.knn import IvfBuilder, build_ivfpq_index, rotate_rows

    x = _data(n, d, seed) if x is None else x
    A = random_rotation(d, seed + 7) if A is None else A
    y = rotate_rows(A, x)
    rng = np.random.default_rng(seed + 1)
    cent = y[rng.choice(n, nlist, replace=False)]
    b = IvfBuilder(d, nlist)
    b.set_centroids(cent)
    lists = b.assign(y)
    b.close()
    cb = _seed_codebooks(y, cent, lists, M, seed + 2)
    ix = build_ivfpq_index(x, nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb, rotation=A, id_base=id_base)
    return x, y, A, cent, cb, ix


def _encode_in_chunks(res, cb, step=500):
    out = [np_encode(res[o:o + step], cb) for o in range(0, len(res), step)]
    return np.concatenate([c for c, _ in out]), np.concatenate([dd for _, dd in out])


# ------------------------------------------------------------------------------------------------ 1. the row-rotation kernel
@pytest.mark.parametrize("d,n", ROT_CASES)
def test_rotation_kernel(d, n):
    """Every output is fp16(y64 + e) with |e| <= 2e-7 (test_opq_cpu.rotation_band: fp16(y64) or, within the band of a midpoint, its
    neighbour), at most 1 % differ from fp16(y64); rows beyond n are not written; A = I returns the input bit for bit."""
    import torch

    from clip_retrieval_amd.knn import rotate_rows, rotate_rows_device

    x, A = unit_rows(n, d, 100 + d + n), random_rotation(d, d)
    xt = torch.from_numpy(x).cuda()
    guard = 3
    yt = torch.full((n + guard, d), 7.0, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    rotate_rows_device(A, xt.data_ptr(), n, yt.data_ptr())
    y = yt.cpu().numpy()
    assert (y[n:] == 7.0).all(), "rows beyond n were written"
    share, worst, outside = rotation_band(y[:n], A, x)
    print(f"d={d} n={n}: kernel: {share:.2e} of the outputs differ from fp16(y64), largest error before rounding {worst:.2e}")
    assert outside == 0 and worst <= BAND, (outside, worst)
    assert share <= CAP, share
    # the identity: bit for bit (a zero sum is +0: an input of -0 comes back as +0)
    same = rotate_rows(np.eye(d, dtype=np.float32), x)
    assert np.array_equal(same.view(np.uint16), np.where(x == 0, np.float16(0), x).view(np.uint16))


# ------------------------------------------------------------------------------------------------ 2. search parity
@pytest.mark.parametrize("d,M,nprobe,B,k", CASES)
def test_search_parity_rotated(d, M, nprobe, B, k):
    n, nlist = 5000, 96
    nprobe = nlist if nprobe == "nlist" else nprobe
    x, y, A, cent, cb, ix = _rotated_index(n, d, nlist, M, nprobe, seed=d + M)
    assert ix.pq_m == M and ix.ntotal == n and ix.nlist == nlist
    assert np.array_equal(ix.pq_rotation(), A)
    codes, lists = ix.pq_codes()
    assert np.array_equal(lists, ix.ivf_lists)
    want, dist = _encode_in_chunks(y.astype(np.float32) - cent[lists].astype(np.float32), cb)
    assert codes_match(codes, want, dist), f"d={d} M={M}: {(codes != want).sum()} codes differ beyond near-ties"
    q = _queries(B, d, seed=B + k, x=x)
    D, I = ix.search(q, k)
    Do, Io, amb = np_adc_search((q.astype(np.float64) @ A.astype(np.float64).T).astype(np.float32), cent, cb, codes, lists, 0, nprobe, k)
    assert amb.mean() < 0.5
    _check(D, I, Do, Io, amb, f"rotated d={d} M={M} nprobe={nprobe} B={B} k={k}")
    ix.close()


# ------------------------------------------------------------------------------------------------ 3. a permutation
def test_permutation_equals_plain_index_of_permuted_rows():
    """A permutation matrix is exact in every precision: D bit for bit and I equal to a plain IVF-PQ index built from the permuted
    rows and searched with the permuted queries (same centroids, same codebooks)."""
    from clip_retrieval_amd.knn import build_ivfpq_index

    n, d, nlist, M, nprobe = 4000, 768, 32, 64, 8
    perm = np.random.default_rng(5).permutation(d)
    P = np.zeros((d, d), np.float32)
    P[np.arange(d), perm] = 1.0  # y = P x: y_j = x_perm[j]
    x, y, _, cent, cb, ix = _rotated_index(n, d, nlist, M, nprobe, seed=13, A=P)
    assert np.array_equal(y, x[:, perm])
    plain = build_ivfpq_index(np.ascontiguousarray(x[:, perm]), nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb)
    assert plain.pq_rotation() is None
    c0, l0 = ix.pq_codes()
    c1, l1 = plain.pq_codes()
    assert np.array_equal(l0, l1) and np.array_equal(c0, c1)
    for B, k in ((1, 40), (33, 64), (256, 10)):
        q = _queries(B, d, seed=B, x=x)
        D0, I0 = ix.search(q, k)
        D1, I1 = plain.search(np.ascontiguousarray(q[:, perm]), k)
        assert np.array_equal(I0, I1) and np.array_equal(D0.view(np.uint32), D1.view(np.uint32)), (B, k)
    ix.close()
    plain.close()


# ------------------------------------------------------------------------------------------------ 4. reconstruction
def test_reconstruct_is_in_the_original_space():
    d, M = 768, 64
    x, _, A, cent, cb, ix = _rotated_index(3000, d, 32, M, 8, seed=5)
    codes, lists = ix.pq_codes()

    def expect(ids):
        dec = cb[np.arange(M)[None, :], codes[ids]].reshape(len(ids), d).astype(np.float64)
        return (cent[lists[ids]].astype(np.float64) + dec) @ A.astype(np.float64)  # A^T applied to rows

    ids = np.array([0, 17, 2999, 1234, -1], dtype=np.int64)
    R = ix.reconstruct_batch(ids)
    assert np.array_equal(R[4].view(np.uint32), np.full(d, 0xFFFFFFFF, np.uint32))
    assert np.abs(R[:4] - expect(ids[:4])).max() <= 1e-5
    q = _queries(4, d, 1, x)
    D, I, R = ix.search_and_reconstruct(q, 64)
    assert (I >= 0).all()
    assert np.abs(R.reshape(-1, d) - expect(I.reshape(-1))).max() <= 1e-5
    D1, I1, R1, _ = ix.search_dedup(q[:1], 40, want_r=True)
    assert np.array_equal(I1[0], I[0, :40])
    assert np.abs(R1[0] - expect(I1[0])).max() <= 1e-5
    ix.close()
    # fewer rows than k in the probed lists: -1 results reconstruct to 0xFF bytes
    x, _, A, cent, cb, ix = _rotated_index(300, 512, 16, 32, 1, seed=6)
    D, I, R = ix.search_and_reconstruct(_queries(3, 512, 2, x), 64)
    assert (I < 0).any()
    assert (R[I < 0].view(np.uint32) == 0xFFFFFFFF).all() and np.isfinite(R[I >= 0]).all()
    ix.close()


# ------------------------------------------------------------------------------------------------ 5. entry points
def test_entry_points_agree_with_batched_search():
    import torch

    x, _, _, _, _, ix = _rotated_index(4000, 512, 32, 32, 8, seed=9)
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
    ix.close()


def test_two_shards_on_one_gpu():
    from clip_retrieval_amd.knn import IvfBuilder, ShardedMi355xIndex, build_ivfpq_index, rotate_rows

    n, d, nlist, M, nprobe = 6000, 768, 48, 32, 6
    x = _data(n, d, 21)
    A = random_rotation(d, 22)
    y = rotate_rows(A, x)
    cent = y[np.random.default_rng(2).choice(n, nlist, replace=False)]
    b = IvfBuilder(d, nlist)
    b.set_centroids(cent)
    lists = b.assign(y)
    b.close()
    cb = _seed_codebooks(y, cent, lists, M, 3)
    cut = [0, 2500, n]
    whole = build_ivfpq_index(x, nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb, rotation=A)
    shards = [build_ivfpq_index(x[cut[g]:cut[g + 1]], nlist, M, nprobe=nprobe, id_base=cut[g], centroids=cent, codebooks=cb, rotation=A)
              for g in range(2)]
    ix = ShardedMi355xIndex.from_shards(shards, cut[:2])
    q = _queries(20, d, 4, x)
    D0, I0 = whole.search(q, 40)
    D, I = ix.search(q, 40)
    assert np.array_equal(I, I0) and np.array_equal(D, D0)
    ix.close()
    whole.close()


def test_save_delete_embeddings_load(tmp_path):
    import shutil

    from clip_retrieval_amd import knn

    n, d, nlist, M = 5000, 512, 32, 64
    emb = tmp_path / "emb"
    emb.mkdir()
    x = _data(n, d, 31)
    np.save(emb / "img_emb_0.npy", x[:3000])
    np.save(emb / "img_emb_1.npy", x[3000:])
    A = random_rotation(d, 32)
    built = knn.build_ivfpq_index_from_folder(str(emb), nlist, M, nprobe=8, niter=3, pq_niter=3, chunk=2048, rotation=A)
    q = _queries(40, d, 5, x)
    D0, I0 = built.search(q, 40)
    out = str(tmp_path / "idx")
    man = knn.save_index(built, out)
    assert man["opq"] is True
    built.close()
    shutil.rmtree(emb)
    assert sorted(os.listdir(out)) == sorted(["ivf_pq_centroids.npy", "ivf_pq_codebooks.npy", "ivf_pq_codes.npy", "ivf_pq_lists.npy",
                                              "ivf_pq_rotation.npy", knn.IVFPQ_MANIFEST])
    loaded = knn.load_index(out)
    assert np.array_equal(loaded.pq_rotation(), A)
    D1, I1 = loaded.search(q, 40)
    assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
    loaded.close()
    lo, hi = 1000, 4200
    part = knn.load_index(out, row_range=(lo, hi))
    D2, I2 = part.search(q, 64)
    loaded = knn.load_index(out)
    loaded.nprobe = nlist
    part.nprobe = nlist
    Dp, Ip = part.search(q, 64)
    Da, Ia = loaded.search(q, 64)
    for i in range(len(q)):  # the shard's answer = the whole index's answer restricted to its rows (all lists probed)
        keep = (Ia[i] >= lo) & (Ia[i] < hi)
        m = int(keep.sum())
        assert np.array_equal(Ip[i, :m], Ia[i][keep]) and np.array_equal(Dp[i, :m], Da[i][keep])
    assert ((I2 < 0) | ((I2 >= lo) & (I2 < hi))).all()
    part.close()
    loaded.close()
    sharded = knn.load_index(out, devices=[0, 0])
    D3, I3 = sharded.search(q, 40)
    assert np.array_equal(I0, I3) and np.array_equal(D0, D3)
    sharded.close()
    # the flag without the file
    os.remove(os.path.join(out, "ivf_pq_rotation.npy"))
    with pytest.raises(ValueError, match="ivf_pq_rotation.npy is missing"):
        knn.load_index(out)
    # a folder written without a rotation carries neither the file nor the key
    plain = knn._ivfpq_from_codes(np.zeros((4, M), np.uint8), np.zeros(4, np.int32), 0, x[:2], np.zeros((M, 256, d // M), np.float32), M, 1, 0)  # pylint: disable=protected-access
    out2 = str(tmp_path / "idx2")
    man2 = knn.save_index(plain, out2)
    plain.close()
    assert "opq" not in man2 and "ivf_pq_rotation.npy" not in os.listdir(out2)
    with open(os.path.join(out2, knn.IVFPQ_MANIFEST), encoding="utf-8") as f:
        assert "opq" not in json.load(f)


def test_device_build_equals_host_build():
    import ctypes as C

    import torch

    from clip_retrieval_amd.knn import build_ivfpq_index_device

    n, d, nlist, M = 7000, 768, 24, 64
    x, _, A, cent, cb, host = _rotated_index(n, d, nlist, M, 4, seed=41)
    xd = torch.from_numpy(x).cuda()

    def fill_rows(dst, row0, count, stride):  # device rows -> dst, completed on return
        src = xd[row0:row0 + count * stride:stride][:count].contiguous()
        torch.cuda.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src.data_ptr()), src.numel() * 2, 3) == 0  # device to device
        torch.cuda.synchronize()  # (a device-to-device hipMemcpy does not wait on the host: without this the copy is not "completed on return")

    dev, stats = build_ivfpq_index_device(fill_rows, n, d, nlist, M, nprobe=4, centroids=cent, codebooks=cb, chunk=3000, rotation=A)
    c0, l0 = host.pq_codes()
    c1, l1 = dev.pq_codes()
    assert np.array_equal(l0, l1) and np.array_equal(c0, c1)
    assert np.array_equal(dev.pq_rotation(), A)
    assert stats["rotate_s"] > 0 and stats["bytes_per_row"] == M + 12
    q = _queries(16, d, 3, x)
    D0, I0 = host.search(q, 40)
    D1, I1 = dev.search(q, 40)
    assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
    host.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import Mi355xIndex, ShardedMi355xIndex, build_ivf_index

    d = 512
    A = random_rotation(d, 1)
    cb = np.zeros((16, 256, d // 16), np.float32)
    e = Mi355xIndex(d)
    with pytest.raises(HipLibraryError, match="after knnx_ivfpq_set_quantizer and before knnx_ivf_begin"):
        e.set_pq_rotation(A)  # a flat index
    assert e.pq_rotation() is None
    e.set_pq_quantizer(16, cb)
    bad = A.copy()
    bad[0] *= 1.01
    with pytest.raises(HipLibraryError, match="not orthonormal"):
        e.set_pq_rotation(bad)
    with pytest.raises(HipLibraryError, match="not orthonormal"):
        e.set_pq_rotation(np.zeros((d, d), np.float32))
    assert e.pq_rotation() is None
    e.set_pq_rotation(A)
    assert np.array_equal(e.pq_rotation(), A)
    e.close()
    x = _data(1000, d, 1)
    flat = build_ivf_index(x, 8, nprobe=2, niter=2)
    with pytest.raises(HipLibraryError, match="after knnx_ivfpq_set_quantizer and before knnx_ivf_begin"):
        flat.set_pq_rotation(A)  # an IVF-Flat index
    flat.close()
    x, _, _, cent, cb, ix = _rotated_index(1000, d, 8, 16, 2, seed=1, A=A)
    with pytest.raises(HipLibraryError, match="after knnx_ivfpq_set_quantizer and before knnx_ivf_begin"):
        ix.set_pq_rotation(A)  # after knnx_ivf_begin / knnx_ivf_end
    # shards with different rotations, and a mix of rotated and plain
    _, _, _, _, _, other = _rotated_index(1000, d, 8, 16, 2, seed=1, A=random_rotation(d, 2), id_base=1000)
    with pytest.raises(HipLibraryError, match="different rotations"):
        ShardedMi355xIndex.from_shards([ix, other], [0, 1000])
    from clip_retrieval_amd.knn import build_ivfpq_index
    plain = build_ivfpq_index(x, 8, 16, nprobe=2, centroids=cent, codebooks=cb, id_base=1000)
    with pytest.raises(HipLibraryError, match="different rotations"):
        ShardedMi355xIndex.from_shards([ix, plain], [0, 1000])
    for i in (ix, other, plain):
        i.close()


# ------------------------------------------------------------------------------------------------ 7. training
def test_train_opq():
    """train_opq on 6 000 rows whose first 16 columns are heavy (test_opq_cpu.heavy_rows: corpus kind 2 with 13 more columns scaled;
    kind 2 alone leaves a numpy OPQ nothing to gain), d = 512, M = 32: orthonormal to 1e-4, the same bytes from the same seed, a
    smaller quantisation error than plain PQ with the same total number of Lloyd iterations, recall@10 at nprobe = nlist not below a
    numpy OPQ of the same recipe minus 0.03."""
    from clip_retrieval_amd.knn import PqBuilder, build_ivfpq_index, rotate_rows, train_ivf_centroids, train_opq, train_pq_codebooks

    n, d, nlist, M, niter, pq_niter = 6000, 512, 16, 32, 4, 4
    x = heavy_rows(n, d, 7)
    A = train_opq(x, M, niter=niter, pq_niter=pq_niter, seed=0)
    assert A.shape == (d, d) and A.dtype == np.float32
    assert np.abs(A.astype(np.float64) @ A.astype(np.float64).T - np.eye(d)).max() <= 1e-4
    assert np.array_equal(A.view(np.uint32), train_opq(x, M, niter=niter, pq_niter=pq_niter, seed=0).view(np.uint32))
    A_np = np_opq(x, M, niter, pq_niter, 0)

    def pq_error(rows, iters):
        """codebooks by the device trainer on `rows` (one list, zero centroid), error measured with np_encode on the host"""
        pb = PqBuilder(d, M)
        pb.set_sample(rows, np.zeros(n, np.int32), np.zeros((1, d), np.float16))
        cb = train_pq_codebooks(pb, niter=iters, seed=3)
        pb.close()
        r = rows.astype(np.float32)
        codes, _ = _encode_in_chunks(r, cb)
        return float(((r - cb[np.arange(M)[None, :], codes].reshape(n, d)) ** 2).sum(1).mean())

    e_opq, e_pq = pq_error(rotate_rows(A, x), pq_niter), pq_error(x, pq_niter * (niter + 1))
    print(f"quantisation error: OPQ {e_opq:.5f}, plain PQ {e_pq:.5f}")
    assert e_opq < e_pq
    q = _queries(64, d, 8, x)
    exact = np.argsort(-(q @ x.astype(np.float32).T), axis=1)[:, :10]

    def recall(rot):
        y = rotate_rows(rot, x)
        cent = train_ivf_centroids(y, nlist, niter=4, seed=0)
        ix = build_ivfpq_index(x, nlist, M, nprobe=nlist, centroids=cent, pq_niter=pq_niter, seed=3, rotation=rot)
        _, I = ix.search(q, 10)
        ix.close()
        return np.mean([len(set(a) & set(b)) / 10 for a, b in zip(I, exact)])

    r_dev, r_np = recall(A), recall(A_np)
    print(f"recall@10: device OPQ {r_dev:.3f}, numpy OPQ {r_np:.3f}")
    assert r_dev >= r_np - 0.03, (r_dev, r_np)
