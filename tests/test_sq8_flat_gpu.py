"""Flat SQ8 (include/knnx.h "Flat SQ8"): one code byte per dimension in id order, searched by the IVF-SQ8 list scan (1 .. 32 queries a
step) and by the one-pass batch scan knn_sq_rq_scan_kernel (larger steps; KNNX_RQ_MIN_ROWS lowered so that small indexes take it).
The reference is float64 numpy on the index's own codes: decode vmin + (code + 0.5) * step, dot, stable sort by (-score, id).
Largest score error observed on an MI355X: see the docstring of test_search_parity."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL, GAP = 1e-5, 2e-5  # the bound tests/test_ivfsq_gpu.py holds IVF-SQ8 scores to; the near-tie width of the id comparison


@pytest.fixture(autouse=True)
def small_batches(monkeypatch):
    monkeypatch.setenv("KNNX_RQ_MIN_ROWS", "0")  # read by knnx_create


def _rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)


def _ranges(x):
    xf = x.astype(np.float32)
    return xf.min(0), xf.max(0) - xf.min(0)


def _encode(x, vmin, vdiff):
    """numpy's encode of fp16 rows: the contract's two roundings in float32."""
    scale = np.where(vdiff == 0, np.float32(0), np.float32(255) / np.where(vdiff == 0, np.float32(1), vdiff)).astype(np.float32)
    t = (x.astype(np.float32) - vmin) * scale
    return np.where(t >= 0, np.minimum(t, 255), 0).astype(np.int32).astype(np.uint8)


def _decode32(codes, vmin, vdiff):
    return (codes.astype(np.float32) + np.float32(0.5)) * (vdiff / np.float32(255)) + vmin


def _reference(codes, vmin, vdiff, q, k):
    dec = vmin.astype(np.float64) + (codes.astype(np.float64) + 0.5) * (vdiff / np.float32(255)).astype(np.float64)
    S = q.astype(np.float64) @ dec.T
    I = np.argsort(-S, axis=1, kind="stable")[:, :k]
    return S, I


def _index(x, ranges=None, chunks=None):
    from clip_retrieval_amd.knn import Mi355xIndex

    ix = Mi355xIndex(x.shape[1], coalesce=False)
    ix.set_sq8_quantizer(*(ranges or _ranges(x)))
    o = 0
    for c in chunks or [x.shape[0]]:
        ix.add(x[o:o + c])
        o += c
    return ix


def _check(ix, codes, vmin, vdiff, q, k):
    """scores within TOL of the float64 score of the returned id; ids = the reference's, up to near-ties of the boundary"""
    D, I = ix.search(q, k)
    S, Iref = _reference(codes, vmin, vdiff, q, k)
    n = codes.shape[0]
    kk = min(k, n)
    assert (I[:, kk:] == -1).all() and (D[:, kk:] == np.finfo(np.float32).min).all()
    err = np.abs(D[:, :kk] - np.take_along_axis(S, I[:, :kk], 1)).max()
    print(f"largest score error {err:.3g}")
    assert err <= TOL
    # where a position holds another id than the reference's (a swap, or the boundary), the two float64 scores are a near-tie
    diff = I[:, :kk] != Iref[:, :kk]
    gap = np.abs(np.take_along_axis(S, I[:, :kk], 1) - np.take_along_axis(S, Iref[:, :kk], 1))
    assert (gap[diff] < GAP).all(), f"ids differ from the reference beyond a near-tie at {np.argwhere(diff)[:5].tolist()}"
    return D, I


@pytest.mark.parametrize("d", [256, 768, 1280, 1100])
def test_codes_and_decode_bit_for_bit(d):
    n = 1037  # 32 tiles + 13 rows
    x = _rows(n, d, 1)
    x[:, 5] = x[0, 5]  # a column with vdiff = 0
    vmin, vdiff = _ranges(x[1:])  # row 0 is not part of the training: its extremes lie outside [vmin, vmin + vdiff] ...
    x[0, 7], x[0, 9] = np.float16(3.0), np.float16(-3.0)  # ... and these certainly do
    ix = _index(x, (vmin, vdiff))
    want = _encode(x, vmin, vdiff)
    assert ix.is_sq8 and ix.ntotal == n
    assert np.array_equal(ix.sq8_codes(), want)
    ids = np.array([0, 31, 32, 1036])
    assert np.array_equal(ix.reconstruct_batch(ids), _decode32(want[ids], vmin, vdiff))


_N = 4133  # 129 tiles + 5 rows
_CORPUS = {}


def _corpus(d):
    """rows, codes, ranges, 300 queries without a near-tie inside any top-64 of the float64 reference (asserted on the CPU), the index"""
    if d not in _CORPUS:
        x = _rows(_N, d, 2)
        vmin, vdiff = _ranges(x)
        codes = _encode(x, vmin, vdiff)
        # queries: those of a pool whose float64 top-65 has no two neighbours closer than GAP (random unit rows at d = 1280 leave about
        # one in sixty), repeated up to 300
        pool = _rows(4000, d, 3).astype(np.float32)
        S, I = _reference(codes, vmin, vdiff, pool, 65)
        top = np.take_along_axis(S, I, 1)
        q = pool[(top[:, :-1] - top[:, 1:]).min(1) >= GAP][:300]
        assert q.shape[0] >= 64, "test bug: too few queries without a near-tie inside their top-64; enlarge the pool"
        q = q[np.arange(300) % q.shape[0]]
        S, I = _reference(codes, vmin, vdiff, q, 65)
        top = np.take_along_axis(S, I, 1)
        assert (top[:, :-1] - top[:, 1:]).min() >= GAP, "test bug: the corpus has a near-tie inside a top-64"
        _CORPUS[d] = (x, codes, vmin, vdiff, q, _index(x, (vmin, vdiff)))
    return _CORPUS[d]


@pytest.mark.parametrize("B", [1, 32, 33, 128, 129, 300])
@pytest.mark.parametrize("k", [1, 40, 64])
@pytest.mark.parametrize("d", [256, 768, 1280])
def test_search_parity(d, k, B):
    """B <= 32: the list scan; B >= 33: the batch kernel (steps of 128 at d = 256, of 64 at d = 768 and 1280), B = 129 and 300 cut into
    passes.  Largest score error observed over all cases on an MI355X: 2.1e-7 (DESIGN 4.8 "Flat SQ8")."""
    x, codes, vmin, vdiff, q, ix = _corpus(d)
    assert np.array_equal(ix.sq8_codes(), codes)
    _check(ix, codes, vmin, vdiff, q[:B], k)


def test_batch_kernel_corners():
    d, k = 768, 64
    # fewer rows than k: two tiles, padded results
    x = _rows(33, d, 4)
    vmin, vdiff = _ranges(x)
    _check(_index(x), _encode(x, vmin, vdiff), vmin, vdiff, _rows(40, d, 5).astype(np.float32), k)
    # zero queries, 200 identical rows in different tiles, a best row at the very end of the arena
    x = _rows(_N, d, 6)
    dup = np.arange(200) * 20 + 3
    x[dup] = x[dup[0]]
    q = _rows(48, d, 7).astype(np.float32)
    q[:16] = 0
    q[16] = x[dup[0]].astype(np.float32)
    x[-1] = (q[17] * 0.9).astype(np.float16)
    vmin, vdiff = _ranges(x)
    vmin[:] = -vdiff / 2  # symmetric ranges: b_q of the zero query is exactly 0
    codes = _encode(x, vmin, vdiff)
    ix = _index(x, (vmin, vdiff))
    D, I = ix.search(q, k)
    assert (D[:16] == 0).all() and (I[:16] == np.arange(k)).all()
    assert np.array_equal(I[16, :k], dup[:k]) and (D[16, :k] == D[16, 0]).all()  # ties by id across workgroups and the merge
    assert I[17, 0] == _N - 1
    S, _ = _reference(codes, vmin, vdiff, q, k)
    assert np.abs(D - np.take_along_axis(S, I, 1)).max() <= TOL


def test_growth_persistence_and_refusals(tmp_path):
    import torch
    from clip_retrieval_amd.knn import HipLibraryError, Mi355xIndex, build_ivfsq_index, load_index, save_index

    d = 1280
    x, codes, vmin, vdiff, q, _ = _corpus(d)
    ix = _index(x, (vmin, vdiff), chunks=[1000, 37, 3096])  # regrowth, a chunk ending mid-tile
    assert np.array_equal(ix.sq8_codes(), codes)
    D, I = _check(ix, codes, vmin, vdiff, q[:70], 40)
    save_index(ix, str(tmp_path))
    ix2 = load_index(str(tmp_path))
    assert ix2.is_sq8 and np.array_equal(ix2.sq8_codes(), codes)
    D2, I2 = ix2.search(q[:70], 40)
    assert np.array_equal(D, D2) and np.array_equal(I, I2)
    ix3 = Mi355xIndex(d)
    ix3.set_sq8_quantizer(vmin, vdiff)
    t = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    ix3.add_sq8_device_rows(t.data_ptr(), x.shape[0])
    assert np.array_equal(ix3.sq8_codes(), codes)
    # KNNX_E_STATE: a non-empty index, an IVF index
    for bad in (ix, build_ivfsq_index(x[:600, :256].copy(), 4, niter=1)):
        with pytest.raises(HipLibraryError, match="KNNX_E_STATE|flat SQ8 quantizer is set once"):
            bad.set_sq8_quantizer(*((vmin, vdiff) if bad is ix else (vmin[:256], vdiff[:256])))
    for call in (lambda: ix.range_search(q[:2], 0.5), lambda: ix.search(q[:2], 65)):
        with pytest.raises(HipLibraryError, match="flat SQ8"):
            call()
    D3, I3 = ix.search(q[:70], 40)
    assert np.array_equal(D, D3) and np.array_equal(I, I3)
