"""IVF-SQ8 at width 1280 (ViT-bigG/14 embeddings): the code scan whose u fragments are split between the LDS and registers, in its
top-k and its threshold mode, and the layers around it, against the numpy restatement of test_ivfsq_cpu.py on the crafted index of
test_ivfsq_gpu.py (24 lists of 0, 1, 31, 32, 33, ... 700 rows, a constant column, rows outside the trained ranges)."""
import numpy as np
import pytest

from test_ivfsq_cpu import np_ranges, np_sq_decode, np_sq_encode, np_sq_scores, np_sq_search
from test_ivfsq_gpu import DUP, N, NLIST, _check, _index, _queries
from test_ivfsq_threshold_gpu import _check_range

pytestmark = pytest.mark.gpu
D = 1280


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# (nprobe, k, B): every nprobe {1, 5, 24}, k {1, 40, 64}, B {1, 32, 33, 300} appears; the queries are _queries(B, D, seed = B + k) as at
# the other widths -- with np_sq_search alone the share of ambiguous probe sets of these six cases is 0 (checked without a GPU)
@pytest.mark.parametrize("nprobe,k,B", [(24, 40, 1), (1, 64, 32), (5, 1, 300), (24, 64, 33), (5, 40, 33), (1, 1, 32)])
def test_search_parity(nprobe, k, B):
    c = _index(D)
    c.ix.nprobe = nprobe
    q = _queries(B, D, seed=B + k, x=c.x)
    Dg, I = c.ix.search(q, k)
    Do, Io, amb = np_sq_search(q, c.cent, c.codes, c.lists, *c.ranges, 0, nprobe, k)
    assert amb.mean() < 0.5
    _check(Dg, I, Do, Io, amb, f"d={D} nprobe={nprobe} k={k} B={B}")


def test_register_held_fragments_are_exact():
    """One list, vmin = 0, vdiff = 255: step = 1, u = q, a score is b_q + 255 * (the sum of q over the row's eight columns).  Row j has
    code 255 in columns 8 j .. 8 j + 7, so every (lane half, k-step) pair of the scan has a row of its own.  Query i has q[c] = 1 + m
    2^-14 with m = 16 (4 c // 5) + 7 t, t = base-3 digit i of the row's number, less one (row j = c // 8): after the scan's scale of
    2^10 the hi part of u is 1024 + 4 c // 5 and the lo part 7 t / 16, the same for the eight columns of a row.  The digits of two rows
    differ in some query, and no row has all five zero: a lo fragment that is dropped, or swapped with or read in place of another
    k-step's or the other lane half's, moves some score of rows 116 .. 159 (k-steps 58 .. 79) by at least 0.6226 (a drop: 255 * 8 * (7 /
    16) / 1024 = 0.8716).  The largest score is 5032.4, the bar 1e-5 of it = 0.05032: a twelfth of that.  (Figures from the
    restatement and the fp16 split of 1024 q, on the CPU.)  The top-k mode answers rows 96 .. 159 (the scores rise with j), the
    threshold mode all 160."""
    from clip_retrieval_amd import knn

    j = np.arange(D) // 8
    t = np.stack([((j + (j >= 121)) // 3**i) % 3 - 1 for i in range(5)])  # (121 = 11111 in base 3 would be five zeros: skipped)
    q = (1 + (16 * (4 * np.arange(D) // 5) + 7 * t) * 2.0**-14).astype(np.float32)
    codes = np.zeros((160, D), np.uint8)
    codes[j, np.arange(D)] = 255
    ranges = (np.zeros(D, np.float32), np.full(D, 255, np.float32))
    cent = np.ones((1, D), np.float16)
    ix = knn._ivfsq_from_codes(codes, np.zeros(160, np.int32), 0, cent, ranges, 1, 0)  # pylint: disable=protected-access
    want = np_sq_scores(q, codes, *ranges)
    bar = 1e-5 * want.max()
    Dg, I = ix.search(q, 64)
    assert np.array_equal(I, np.tile(np.arange(159, 95, -1), (5, 1)))
    err = np.abs(Dg - np.take_along_axis(want, I, 1)).max()
    ix.sq_threshold_scan = True
    Dt, It = ix.search(q, 160)
    assert np.array_equal(It, np.tile(np.arange(159, -1, -1), (5, 1)))
    err_t = np.abs(Dt - np.take_along_axis(want, It, 1)).max()
    print(f"largest score {want.max():.1f}, bar {bar:.4g}; max error top-k {err:.3g}, threshold {err_t:.3g}")
    assert err <= bar and err_t <= bar and np.array_equal(_bits(Dt[:, :64]), _bits(Dg))
    ix.close()


def test_topk_and_threshold_modes_agree():
    """range_search (a few hundred hits) and k = 100 against numpy; the first 64 of k = 100 are the k = 64 search, bit for bit."""
    c = _index(D)
    c.ix.nprobe = 5
    q = _queries(33, D, seed=40, x=c.x)
    Do, Io, amb = np_sq_search(q, c.cent, c.codes, c.lists, *c.ranges, 0, 5, N + 10)
    assert amb.mean() < 0.5
    D64, I64 = c.ix.search(q, 64)
    c.ix.sq_threshold_scan = True
    try:
        thr = float(np.sort(Do[~amb].ravel())[-400])
        lims, Dr, Ir = c.ix.range_search(q, thr)
        D100, I100 = c.ix.search(q, 100)
    finally:
        c.ix.sq_threshold_scan = False
    _check_range(lims, Dr, Ir, Do, Io, amb, thr, "range")
    _check(D100, I100, Do[:, :100], Io[:, :100], amb, "k=100")
    assert np.array_equal(I100[:, :64], I64) and np.array_equal(_bits(D100[:, :64]), _bits(D64))


def test_codes_ranges_and_decode():
    """sq_codes = np_sq_encode byte for byte (the constant column, clamped rows); reconstruct = np_sq_decode and the column min / max of
    1037 x 1280 rows = numpy's, bit for bit."""
    import torch

    from clip_retrieval_amd.knn import train_sq_ranges

    c = _index(D)
    codes, lists = c.ix.sq_codes()
    assert np.array_equal(lists, c.lists) and np.array_equal(codes, c.codes)
    assert (c.codes == 0).any() and (c.codes == 255).any() and (c.codes[:, 7] == 0).all()
    ids = np.array([0, 17, N - 1, 1234, 10], dtype=np.int64)
    assert np.array_equal(_bits(c.ix.reconstruct_batch(ids)), _bits(np_sq_decode(c.codes, *c.ranges)[ids]))
    x = (0.1 * np.random.default_rng(1037).standard_normal((1037, D))).astype(np.float16)
    x[1036, 1279], x[1036, 1024] = 9.0, -9.0  # the extremes in the last, partial group of rows, in the fifth column of a thread
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    for got in (train_sq_ranges(x, chunk=500), train_sq_ranges(xd.data_ptr(), 1037, D)):
        assert np.array_equal(_bits(np.stack(got)), _bits(np.stack(np_ranges(x))))


def test_public_layers_at_a_padded_width(tmp_path):
    """A user width of 1100 (padded to 1280): build, save / load, append + remove against a fresh build, the filtered search."""
    from clip_retrieval_amd import knn

    d = 1100
    c = _index(D)
    x, cent, ranges = c.x[:, :d].copy(), c.cent[:, :d].copy(), (c.ranges[0][:d].copy(), c.ranges[1][:d].copy())
    ix = knn.build_ivfsq_index(x, NLIST, nprobe=5, centroids=cent, ranges=ranges)
    q = _queries(33, d, seed=2, x=x)
    D0, I0 = ix.search(q, 40)
    knn.save_index(ix, str(tmp_path / "idx"))
    loaded = knn.load_index(str(tmp_path / "idx"))
    D1, I1 = loaded.search(q, 40)
    loaded.close()
    assert np.array_equal(I0, I1) and np.array_equal(_bits(D0), _bits(D1))
    ix.nprobe = NLIST  # the planted near-copies of row DUP[0]: dropped by the device filter as by numpy on the decoded rows
    Df, If, drop, stats = ix.search_filtered(x[DUP[0]:DUP[0] + 1].astype(np.float32), 40, dedup_thr=0.94)
    Ds, Is = ix.search(x[DUP[0]:DUP[0] + 1].astype(np.float32), 40)
    r = np_sq_decode(np_sq_encode(x[Is[0]], *ranges), *ranges).astype(np.float64)
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    s = np.triu(r @ r.T, 1)
    assert np.abs(s[s > 0.5] - 0.94).min() > 1e-5, "test bug: a pair at the dedup threshold"
    want = np.array([(s[:i, i] > 0.94).any() for i in range(40)])  # (the near-copies link to the best-ranked of them directly)
    assert np.array_equal(If, Is) and np.array_equal(_bits(Df), _bits(Ds)) and want.sum() >= 3 and np.array_equal(drop.astype(bool), want)
    ix.nprobe = 5
    extra = c.x[:100, :d][::-1].copy()
    ix.ivf_append(extra)
    rows = np.concatenate([x, extra])[ix.ivf_remove(np.arange(0, N + 100, 35)[:100])]
    fresh = knn.build_ivfsq_index(rows, NLIST, nprobe=5, centroids=cent, ranges=ranges)
    for a, b in zip(ix.search_and_reconstruct(q, 40), fresh.search_and_reconstruct(q, 40)):
        assert a.tobytes() == b.tobytes()
    fresh.close()
    ix.close()


def test_refusals_that_remain():
    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.knn import Mi355xIndex

    pq = Mi355xIndex(D)
    with pytest.raises(HipLibraryError, match=r"code -5\): IVF-PQ takes d <= 1024"):
        pq.set_pq_quantizer(16, np.zeros(256 * D, np.float32))
    pq.close()
    with pytest.raises(HipLibraryError, match=r"code -5\).*<= 1280"):
        Mi355xIndex(1536)
