"""OPQ with d_out > d_in in front of IVF-PQ (faiss IndexPreTransform(OPQMatrix(d_in, M, d_out), IndexIVFPQ(..., d_out, ...)); the
reference notebook's OPQ256_768 on 512-d rows): the row kernel for rectangular matrices, bit equality with the square d_out index over
zero-padded rows (every extra term of every summation chain is an exact zero), parity with the numpy restatement of
tests/test_ivfpq_gpu.py in the rotated space, rows that come back d_in wide, the refine store, the other configurations, training and
refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from test_ivfpq_gpu import _check, _data, _queries, _seed_codebooks, codes_match, np_adc_search, np_encode
from test_opq_cpu import BAND, CAP, heavy_rows, np_pq_encode, random_rotation, rotation_band, unit_rows
from test_opq_rect_cpu import rect_rotation

pytestmark = pytest.mark.gpu

KNNX_E_ARG, KNNX_E_STATE = -1, -4


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _pad(a, d_out):
    out = np.zeros((a.shape[0], d_out), a.dtype)
    out[:, : a.shape[1]] = a
    return out


def _parts(n, d_in, d_out, nlist, M, seed):
    """Rows, a rectangular rotation and a quantiser of the rotated space: random rotated rows as centroids, codebooks from residual
    sub-vectors of random rows, y = the device's own rotated rows.  -> x [n, d_in], y [n, d_out], A_sq, A, cent [nlist, d_out], cb, lists"""
    from clip_retrieval_amd.knn import IvfBuilder, rotate_rows

    x = _data(n, d_in, seed)
    A_sq, A = rect_rotation(d_in, d_out, seed + 7)
    y = rotate_rows(A, x)
    assert y.shape == (n, d_out) and y.dtype == np.float16
    cent = y[np.random.default_rng(seed + 1).choice(n, nlist, replace=False)]
    b = IvfBuilder(d_out, nlist)
    b.set_centroids(cent)
    lists = b.assign(y)
    b.close()
    return x, y, A_sq, A, cent, _seed_codebooks(y, cent, lists, M, seed + 2), lists


def _codes_are_the_numpy_encoding(codes, y, cent, lists, cb):
    res = y.astype(np.float32) - cent[lists].astype(np.float32)
    bad = np.flatnonzero((codes != np_pq_encode(res, cb)).any(1))
    assert len(bad) <= 600, len(bad)  # the full distance array is formed for the rows that differ only
    for o in range(0, len(bad), 100):
        want, dist = np_encode(res[bad[o:o + 100]], cb)
        assert codes_match(codes[bad[o:o + 100]], want, dist), "codes differ beyond near-ties"


def _tiles(lists, nlist):
    return int(((np.bincount(lists, minlength=nlist) + 31) // 32).sum())


# ------------------------------------------------------------------------------------------------ 1. the row kernel
@pytest.mark.parametrize("n", [1, 33, 5000])
@pytest.mark.parametrize("d_in,d_out", [(512, 768), (256, 1024), (768, 1024)])
def test_rotation_kernel_rect(d_in, d_out, n):
    """Every output is fp16(y64 + e) with |e| <= 2e-7, at most 1 % differ from fp16(y64) (test_opq_cpu.rotation_band; float32 numpy on
    the same inputs: test_opq_rect_cpu); the 3 guard rows after n are untouched; a column-selection embedding returns x scattered into
    zeros bit for bit."""
    import torch

    from clip_retrieval_amd.knn import rotate_rows, rotate_rows_device

    x = unit_rows(n, d_in, 100 + d_in + d_out + n)
    _, A = rect_rotation(d_in, d_out)
    xt = torch.from_numpy(x).cuda()
    guard = 3
    yt = torch.full((n + guard, d_out), 7.0, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    rotate_rows_device(A, xt.data_ptr(), n, yt.data_ptr())
    y = yt.cpu().numpy()
    assert (y[n:] == 7.0).all(), "rows beyond n were written"
    share, worst, outside = rotation_band(y[:n], A, x)
    print(f"d_in={d_in} d_out={d_out} n={n}: kernel: {share:.2e} of the outputs differ from fp16(y64), largest error {worst:.2e}")
    assert outside == 0 and worst <= BAND, (outside, worst)
    assert share <= CAP, share
    pos = np.sort(np.random.default_rng(d_in + d_out).choice(d_out, d_in, replace=False))
    E = np.zeros((d_out, d_in), np.float32)
    E[pos, np.arange(d_in)] = 1.0
    want = np.zeros((n, d_out), np.float16)
    want[:, pos] = np.where(x == 0, np.float16(0), x)  # (a zero sum is +0: an input of -0 comes back as +0)
    assert np.array_equal(_bits(rotate_rows(E, x)), _bits(want))


# ------------------------------------------------------------------------------------------------ 2. bit equality with the square path
@pytest.mark.parametrize("M", [64, 256])
def test_bit_equality_with_the_padded_square_index(M):
    """A = the first 512 columns of a 768 rotation.  The rectangular index over x and the square d = 768 index over zero-padded x with
    the same centroids and codebooks hold the same codes and answer with the same D bits and ids; reconstruct gives the square one's
    first 512 columns bit for bit (its other 256 are what A_sq^T makes of them)."""
    from clip_retrieval_amd.knn import build_ivfpq_index, rotate_rows

    n, d, dq, nlist, nprobe = 5000, 512, 768, 64, 8
    x, y, A_sq, A, cent, cb, _ = _parts(n, d, dq, nlist, M, seed=M)
    xp = _pad(x, dq)
    assert np.array_equal(_bits(rotate_rows(A_sq, xp)), _bits(y))
    rect = build_ivfpq_index(x, nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb, rotation=A)
    sq = build_ivfpq_index(xp, nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb, rotation=A_sq)
    assert (rect.d, rect.pq_out_dim, sq.d, sq.pq_out_dim) == (d, dq, dq, dq)
    assert np.array_equal(rect.pq_rotation(), A) and rect.pq_codebooks().shape == (M, 256, dq // M)
    (c0, l0), (c1, l1) = rect.pq_codes(), sq.pq_codes()
    assert np.array_equal(l0, l1) and np.array_equal(c0, c1)
    for B, k in ((1, 40), (33, 64), (256, 10)):
        q = _queries(B, d, seed=B, x=x)
        D0, I0 = rect.search(q, k)
        D1, I1 = sq.search(_pad(q, dq), k)
        assert np.array_equal(I0, I1) and np.array_equal(_bits(D0), _bits(D1)), (B, k)
    ids = np.array([0, 17, n - 1, 1234, -1, 4097], dtype=np.int64)
    R0, R1 = rect.reconstruct_batch(ids), sq.reconstruct_batch(ids)
    assert R0.shape == (len(ids), d) and np.array_equal(_bits(R0), _bits(R1[:, :d]))
    rect.close()
    sq.close()


# ------------------------------------------------------------------------------------------------ 3. numpy parity
@pytest.mark.parametrize("d_in,d_out,M,nprobe,B,k", [(512, 768, 256, 8, 33, 40), (512, 768, 64, "nlist", 256, 64), (256, 512, 32, 1, 1, 1),
                                                      (768, 1024, 128, 80, 300, 40)])
def test_search_parity_rect(d_in, d_out, M, nprobe, B, k):
    from clip_retrieval_amd.knn import build_ivfpq_index

    n, nlist = 5000, 96
    nprobe = nlist if nprobe == "nlist" else nprobe
    x, y, _, A, cent, cb, lists0 = _parts(n, d_in, d_out, nlist, M, seed=d_in + d_out + M)
    ix = build_ivfpq_index(x, nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb, rotation=A)
    assert (ix.pq_m, ix.ntotal, ix.nlist, ix.d, ix.pq_out_dim) == (M, n, nlist, d_in, d_out)
    codes, lists = ix.pq_codes()
    assert np.array_equal(lists, ix.ivf_lists) and np.array_equal(lists, lists0)
    _codes_are_the_numpy_encoding(codes, y, cent, lists, cb)
    q = _queries(B, d_in, seed=B + k, x=x)
    D, I = ix.search(q, k)
    Do, Io, amb = np_adc_search((q.astype(np.float64) @ A.astype(np.float64).T).astype(np.float32), cent, cb, codes, lists, 0, nprobe, k)
    assert amb.mean() < 0.5
    _check(D, I, Do, Io, amb, f"rect d_in={d_in} d_out={d_out} M={M} nprobe={nprobe} B={B} k={k}")
    ix.close()


# ------------------------------------------------------------------------------------------------ 4. rows come back d_in wide
def test_reconstruct_is_in_the_original_space_rect():
    from clip_retrieval_amd.knn import build_ivfpq_index

    d, dq, M, n, nlist = 512, 768, 64, 3000, 32
    x, _, _, A, cent, cb, _ = _parts(n, d, dq, nlist, M, seed=5)
    ix = build_ivfpq_index(x, nlist, M, nprobe=8, centroids=cent, codebooks=cb, rotation=A)
    codes, lists = ix.pq_codes()

    def expect(ids):
        dec = cb[np.arange(M)[None, :], codes[ids]].reshape(len(ids), dq).astype(np.float64)
        return (cent[lists[ids]].astype(np.float64) + dec) @ A.astype(np.float64)  # A^T applied to rows: [.., d_out] -> [.., d_in]

    ids = np.array([0, 17, n - 1, 1234, -1], dtype=np.int64)
    R = ix.reconstruct_batch(ids)
    assert R.shape == (5, d)
    assert np.array_equal(R[4].view(np.uint32), np.full(d, 0xFFFFFFFF, np.uint32))
    assert np.abs(R[:4] - expect(ids[:4])).max() <= 1e-5
    q = _queries(4, d, 1, x)
    D, I, R = ix.search_and_reconstruct(q, 64)
    assert (I >= 0).all() and R.shape == (4, 64, d)
    assert np.abs(R.reshape(-1, d) - expect(I.reshape(-1))).max() <= 1e-5
    D1, I1, R1, _ = ix.search_dedup(q[:1], 40, want_r=True)
    assert np.array_equal(I1[0], I[0, :40]) and R1.shape[-1] == d
    assert np.abs(R1[0] - expect(I1[0])).max() <= 1e-5
    ix.close()
    # fewer rows than k in the probed lists: -1 results reconstruct to 0xFF bytes
    x, _, _, A, cent, cb, _ = _parts(300, 256, 512, 16, 32, seed=6)
    ix = build_ivfpq_index(x, 16, 32, nprobe=1, centroids=cent, codebooks=cb, rotation=A)
    D, I, R = ix.search_and_reconstruct(_queries(3, 256, 2, x), 64)
    assert (I < 0).any() and R.shape == (3, 64, 256)
    assert (R[I < 0].view(np.uint32) == 0xFFFFFFFF).all() and np.isfinite(R[I >= 0]).all()
    ix.close()


# ------------------------------------------------------------------------------------------------ 5. refine store
def test_refine_store_is_d_in_wide():
    """The row arena is tiles x 32 x 512 x 2 bytes, R is f32(x_f16) bit for bit, and the exact scores are those of the zero-padded
    square refine index bit for bit (its 256 extra products are exact zeros at the end of the chains)."""
    from clip_retrieval_amd.knn import build_ivfpq_index

    n, d, dq, nlist, M, nprobe = 5000, 512, 768, 64, 64, 8
    x, _, A_sq, A, cent, cb, lists = _parts(n, d, dq, nlist, M, seed=11)
    rect = build_ivfpq_index(x, nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb, rotation=A, refine=True, k_factor=4)
    sq = build_ivfpq_index(_pad(x, dq), nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb, rotation=A_sq, refine=True, k_factor=4)
    tiles = _tiles(lists, nlist)
    assert rect.pq_arena_bytes() == (tiles * 32 * M, tiles * 32 * d * 2)
    assert sq.pq_arena_bytes() == (tiles * 32 * M, tiles * 32 * dq * 2)
    for B, k in ((1, 40), (33, 64), (256, 10)):
        q = _queries(B, d, seed=B + 1, x=x)
        D0, I0, R0 = rect.search_and_reconstruct(q, k)
        D1, I1 = sq.search(_pad(q, dq), k)
        assert np.array_equal(I0, I1) and np.array_equal(_bits(D0), _bits(D1)), (B, k)
        assert (I0 >= 0).all() and R0.shape == (B, k, d)
        assert np.array_equal(_bits(R0), _bits(x[I0].astype(np.float32)))
    ids = np.array([3, n - 1, -1], dtype=np.int64)
    R = rect.reconstruct_batch(ids)
    assert np.array_equal(_bits(R[:2]), _bits(x[ids[:2]].astype(np.float32))) and (R[2].view(np.uint32) == 0xFFFFFFFF).all()
    rect.close()
    sq.close()


# ------------------------------------------------------------------------------------------------ 6. other configurations
def test_threshold_scan_rect():
    from clip_retrieval_amd.knn import build_ivfpq_index

    n, d, dq, nlist, M = 5000, 512, 768, 32, 64
    x, _, _, A, cent, cb, _ = _parts(n, d, dq, nlist, M, seed=17)
    ix = build_ivfpq_index(x, nlist, M, nprobe=8, centroids=cent, codebooks=cb, rotation=A, threshold_scan=True)
    q = _queries(5, d, 3, x)
    D64, I64 = ix.search(q, 64)
    D200, I200 = ix.search(q, 200)
    assert (I200 >= 0).all()
    assert np.array_equal(I200[:, :64], I64) and np.array_equal(_bits(D200[:, :64]), _bits(D64))
    ix.close()


def test_two_shards_on_one_gpu_rect():
    from clip_retrieval_amd.knn import ShardedMi355xIndex, build_ivfpq_index

    n, d, dq, nlist, M, nprobe = 5000, 512, 768, 48, 32, 6
    x, _, _, A, cent, cb, _ = _parts(n, d, dq, nlist, M, seed=21)
    cut = [0, 2100, n]
    whole = build_ivfpq_index(x, nlist, M, nprobe=nprobe, centroids=cent, codebooks=cb, rotation=A)
    shards = [build_ivfpq_index(x[cut[g]:cut[g + 1]], nlist, M, nprobe=nprobe, id_base=cut[g], centroids=cent, codebooks=cb, rotation=A)
              for g in range(2)]
    ix = ShardedMi355xIndex.from_shards(shards, cut[:2])
    assert ix.d == d
    q = _queries(20, d, 4, x)
    D0, I0, R0 = whole.search_and_reconstruct(q, 40)
    D, I, R = ix.search_and_reconstruct(q, 40)
    assert np.array_equal(I, I0) and np.array_equal(D, D0) and R.shape == (20, 40, d) and np.array_equal(_bits(R), _bits(R0))
    ix.close()
    whole.close()


def test_save_load_round_trip_rect(tmp_path):
    import json
    import shutil

    from clip_retrieval_amd import knn

    n, d, dq, nlist, M = 5000, 512, 768, 32, 256
    emb = tmp_path / "emb"
    emb.mkdir()
    x = _data(n, d, 31)
    np.save(emb / "img_emb_0.npy", x[:3000])
    np.save(emb / "img_emb_1.npy", x[3000:])
    _, A = rect_rotation(d, dq, 32)
    built = knn.build_ivfpq_index_from_folder(str(emb), nlist, M, nprobe=8, niter=3, pq_niter=3, chunk=2048, rotation=A)
    assert (built.d, built.pq_out_dim) == (d, dq) and built.ivf_centroids.shape == (nlist, dq)
    q = _queries(40, d, 5, x)
    D0, I0 = built.search(q, 40)
    out = str(tmp_path / "idx")
    man = knn.save_index(built, out)
    assert man["opq"] is True and man["d"] == d and man["d_out"] == dq
    with open(os.path.join(out, knn.IVFPQ_MANIFEST), encoding="utf-8") as f:
        assert json.load(f)["d_out"] == dq
    assert np.load(os.path.join(out, knn.IVFPQ_ROTATION)).shape == (dq, d)
    # the same index with a refine store: the folder is loaded together with the embeddings and re-encodes them to the saved codes
    ref = knn.build_ivfpq_index_from_folder(str(emb), nlist, M, nprobe=8, chunk=2048, rotation=A, centroids=built.ivf_centroids,
                                            codebooks=built.pq_codebooks(), refine=True, k_factor=2)
    Dr, Ir = ref.search(q, 40)
    out_r = str(tmp_path / "idx_refine")
    assert knn.save_index(ref, out_r)["d_out"] == dq
    ref.close()
    built.close()
    loaded_r = knn.load_index(out_r)
    assert loaded_r.pq_refine and (loaded_r.d, loaded_r.pq_out_dim) == (d, dq)
    D4, I4 = loaded_r.search(q, 40)
    assert np.array_equal(Ir, I4) and np.array_equal(Dr, D4)
    loaded_r.close()
    shutil.rmtree(emb)
    loaded = knn.load_index(out)
    assert (loaded.d, loaded.pq_out_dim) == (d, dq) and np.array_equal(loaded.pq_rotation(), A)
    D1, I1 = loaded.search(q, 40)
    assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
    loaded.close()
    lo, hi = 1000, 4200
    part = knn.load_index(out, row_range=(lo, hi))
    D2, I2 = part.search(q, 64)
    assert ((I2 < 0) | ((I2 >= lo) & (I2 < hi))).all() and part.pq_out_dim == dq
    part.close()
    sharded = knn.load_index(out, devices=[0, 0])
    D3, I3 = sharded.search(q, 40)
    assert np.array_equal(I0, I3) and np.array_equal(D0, D3)
    sharded.close()
    # the key without the matching file
    np.save(os.path.join(out, knn.IVFPQ_ROTATION), random_rotation(d, 1))
    with pytest.raises(ValueError, match=rf"must be float32 \[{dq}, {d}\]"):
        knn.load_index(out)


def test_device_build_equals_host_build_rect():
    import torch

    from clip_retrieval_amd.knn import build_ivfpq_index, build_ivfpq_index_device

    n, d, dq, nlist, M = 5000, 512, 768, 24, 64
    x, _, _, A, cent, cb, lists = _parts(n, d, dq, nlist, M, seed=41)
    host = build_ivfpq_index(x, nlist, M, nprobe=4, centroids=cent, codebooks=cb, rotation=A, refine=True)
    xd = torch.from_numpy(x).cuda()

    def fill_rows(dst, row0, count, stride):  # device rows -> dst, completed on return
        src = xd[row0:row0 + count * stride:stride][:count].contiguous()
        torch.cuda.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src.data_ptr()), src.numel() * 2, 3) == 0  # device to device
        torch.cuda.synchronize()  # (a device-to-device hipMemcpy does not wait on the host: without this the copy is not "completed on return")

    dev, stats = build_ivfpq_index_device(fill_rows, n, d, nlist, M, nprobe=4, centroids=cent, codebooks=cb, chunk=2000, rotation=A,
                                          refine=True)
    (c0, l0), (c1, l1) = host.pq_codes(), dev.pq_codes()
    assert np.array_equal(l0, l1) and np.array_equal(c0, c1)
    assert np.array_equal(dev.pq_rotation(), A) and (dev.d, dev.pq_out_dim) == (d, dq)
    tiles = _tiles(lists, nlist)
    assert stats["rotate_s"] > 0 and stats["opq_s"] == 0 and stats["bytes_per_row"] == M + 12 + 2 * d
    assert stats["row_arena_bytes"] == tiles * 32 * d * 2 and stats["code_arena_bytes"] == tiles * 32 * M
    q = _queries(16, d, 3, x)
    D0, I0 = host.search(q, 40)
    D1, I1 = dev.search(q, 40)
    assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
    host.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ 7. training
def test_train_opq_rect():
    """train_opq(d_out=768) on 6 000 rows of width 512 whose first 16 columns are heavy (test_opq_cpu.heavy_rows), M = 32: columns
    orthonormal to 1e-4, and PQ of the rotated rows loses less than PQ of the rows zero-embedded into 768 columns -- which gets the
    Lloyd iterations the OPQ training spent as well."""
    from clip_retrieval_amd.knn import PqBuilder, rotate_rows, train_opq, train_pq_codebooks

    n, d, dq, M, niter, pq_niter = 6000, 512, 768, 32, 4, 4
    x = heavy_rows(n, d, 7)
    A = train_opq(x, M, niter=niter, pq_niter=pq_niter, seed=0, d_out=dq)
    assert A.shape == (dq, d) and A.dtype == np.float32 and A.flags.c_contiguous
    A64 = A.astype(np.float64)
    assert np.abs(A64.T @ A64 - np.eye(d)).max() <= 1e-4

    def pq_error(rows, iters):
        pb = PqBuilder(dq, M)
        pb.set_sample(rows, np.zeros(n, np.int32), np.zeros((1, dq), np.float16))
        cb = train_pq_codebooks(pb, niter=iters, seed=3)
        pb.close()
        r = rows.astype(np.float32)
        return float(((r - cb[np.arange(M)[None, :], np_pq_encode(r, cb)].reshape(n, dq)) ** 2).sum(1).mean())

    e_opq, e_embed = pq_error(rotate_rows(A, x), pq_niter), pq_error(_pad(x, dq), pq_niter * (niter + 1))
    print(f"quantisation error: rectangular OPQ {e_opq:.5f}, zero-embedding {e_embed:.5f}")
    assert e_opq < e_embed


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_rect():
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import Mi355xIndex, ShardedMi355xIndex, build_ivfpq_index, rotate_rows

    d, dq, M = 512, 768, 16
    A_sq, A = rect_rotation(d, dq, 1)
    cb = np.zeros((M, 256, dq // M), np.float32)

    def err(ix):
        return ix._lib.knnx_last_error().decode()  # pylint: disable=protected-access

    # bad widths: KNNX_E_ARG, both widths named; the index stays what it was
    e = Mi355xIndex(d)
    lib, h = e._lib, e._h  # pylint: disable=protected-access
    assert lib.knnx_ivfpq_out_dim(h) == 0  # not an IVF-PQ index (yet)
    for bad in (700, 256, 0, 1280, -768):
        assert lib.knnx_ivfpq_set_out_dim(h, bad) == KNNX_E_ARG
        assert str(bad) in err(e) and str(d) in err(e)
    with pytest.raises(HipLibraryError, match="d_out = 700"):
        e.set_pq_out_dim(700)
    assert lib.knnx_ivfpq_set_out_dim(h, d) == 0 and e.pq_out_dim == d  # d_out == d: accepted, changes nothing
    odd = Mi355xIndex(100)
    with pytest.raises(ValueError, match="d % 256 == 0"):
        odd.set_pq_out_dim(256)
    odd.close()
    # the quantizer follows d_out; set_out_dim after it: KNNX_E_STATE
    e.set_pq_out_dim(dq)
    assert e.pq_out_dim == dq
    with pytest.raises(AssertionError):
        e.set_pq_quantizer(M, np.zeros((M, 256, d // M), np.float32))  # codebooks of the d shape
    e.set_pq_quantizer(M, cb)
    assert lib.knnx_ivfpq_out_dim(h) == dq and lib.knnx_dim(h) == d
    assert lib.knnx_ivfpq_set_out_dim(h, dq) == KNNX_E_STATE and lib.knnx_ivfpq_set_out_dim(h, 1024) == KNNX_E_STATE
    assert "before knnx_ivfpq_set_quantizer" in err(e)
    # knnx_ivf_begin without a rotation: KNNX_E_STATE that says why
    cent = np.zeros((4, dq), np.float16)
    sizes = np.zeros(4, np.int64)
    assert lib.knnx_ivf_begin(h, 4, cent.ctypes.data, sizes.ctypes.data) == KNNX_E_STATE
    assert "rotation" in err(e) and str(dq) in err(e)
    # a [768][768] matrix on a 512 / 768 index: the wrapper refuses the shape, the library what it reads as [768][512]
    with pytest.raises(AssertionError, match=rf"\[{dq}, {d}\]"):
        e.set_pq_rotation(A_sq)
    assert lib.knnx_ivfpq_set_rotation(h, np.ascontiguousarray(A_sq).ctypes.data) == KNNX_E_ARG
    assert "orthonormal columns" in err(e)
    bad = A.copy()
    bad[:, 0] *= 1.01
    with pytest.raises(HipLibraryError, match="orthonormal columns"):
        e.set_pq_rotation(bad)
    bad = A.copy()
    bad[5, 5] = np.nan
    with pytest.raises(HipLibraryError, match="orthonormal columns"):
        e.set_pq_rotation(bad)
    assert e.pq_rotation() is None
    e.set_pq_rotation(A)
    assert np.array_equal(e.pq_rotation(), A)
    e.close()
    # shards of mixed widths: the rectangular index next to the square one of the same d and the same M
    n, nlist = 1000, 8
    x, _, _, A2, cent, cb2, _ = _parts(n, d, dq, nlist, M, seed=3)
    rect = build_ivfpq_index(x, nlist, M, nprobe=2, centroids=cent, codebooks=cb2, rotation=A2)
    square = build_ivfpq_index(x, nlist, M, nprobe=2, centroids=rotate_rows(random_rotation(d, 9), x[:nlist]),
                               codebooks=np.zeros((M, 256, d // M), np.float32), rotation=random_rotation(d, 9), id_base=n)
    assert lib.knnx_ivfpq_set_out_dim(rect._h, dq) == KNNX_E_STATE  # pylint: disable=protected-access  # (an index that has rows and lists)
    with pytest.raises(HipLibraryError, match=rf"d_out = {dq} and {d}"):
        ShardedMi355xIndex.from_shards([rect, square], [0, n])
    # the same widths behind another rotation
    _, other_A = rect_rotation(d, dq, 77)
    other = build_ivfpq_index(x, nlist, M, nprobe=2, centroids=cent, codebooks=cb2, rotation=other_A, id_base=n)
    with pytest.raises(HipLibraryError, match="different rotations"):
        ShardedMi355xIndex.from_shards([rect, other], [0, n])
    for i in (rect, square, other):
        i.close()
