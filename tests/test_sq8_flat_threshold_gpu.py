"""The threshold scan of flat SQ8 on the GPU (Mi355xIndex.sq8_threshold_scan; include/knnx.h "Flat SQ8"): k > 64 and range_search through
the list scan's threshold mode (groups of <= 32 queries) and knn_sq_rq_range_scan_kernel (larger groups), against float64 numpy on the
index's own codes -- the 4 133-row corpus of test_sq8_flat_gpu.py (129 tiles + 5 rows).  That corpus index is shared with tests that
expect the switch OFF: the fixture `on` switches it on and off again."""
import numpy as np
import pytest

from test_sq8_flat_gpu import GAP, TOL, _N, _corpus, _encode, _ranges, _reference, _rows, small_batches  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu
NEAR_MAX = 0.005  # reference hits within TOL of the threshold may fall on either side: at most this share of a case's reference hits
_REF = {}


@pytest.fixture
def on():
    used = []

    def get(d):
        c = _corpus(d)
        c[5].sq8_threshold_scan = True
        used.append(c[5])
        if d not in _REF:  # float64 scores of the first 128 queries against every row, and their full ranking: once per width
            _REF[d] = _reference(c[1], c[2], c[3], c[4][:128], _N)
        return c[4], c[5], _REF[d][0], _REF[d][1]

    yield get
    for ix in used:
        ix.sq8_threshold_scan = False


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("k", [65, 3000, _N + 10])
@pytest.mark.parametrize("B", [1, 33, 70, 128])
@pytest.mark.parametrize("d", [256, 768, 1280])
def test_large_k(on, d, B, k):
    """B = 1: the list route; 33 and 128: the batch kernel; 70: the batch kernel, at d >= 768 plus a tail of 6 on the list route."""
    q, ix, S, Iref = on(d)
    before = ix.sq8_threshold_stats()
    D, I = ix.search(q[:B], k)
    queries, launches, qscans, _ = (a - b for a, b in zip(ix.sq8_threshold_stats(), before))
    assert queries == B and launches >= 1 and qscans >= B
    kk = min(k, _N)
    assert (I[:, kk:] == -1).all() and (D[:, kk:] == np.finfo(np.float32).min).all() and (I[:, :kk] >= 0).all()
    got, want = np.take_along_axis(S[:B], I[:, :kk], 1), np.take_along_axis(S[:B], Iref[:B, :kk], 1)
    err = np.abs(D[:, :kk] - got).max()
    print(f"d={d} B={B} k={k}: {launches} launches, {qscans / B:.2f} scans per query, largest score error {err:.3g}")
    assert err <= TOL
    assert (np.abs(got - want)[I[:, :kk] != Iref[:B, :kk]] < GAP).all()  # another id than the reference's only at a near-tie


@pytest.mark.parametrize("B", [32, 64])
@pytest.mark.parametrize("d", [256, 768])
def test_first_64_of_large_k_are_the_k64_search(on, d, B):
    q, ix, _, _ = on(d)
    D64, I64 = ix.search(q[:B], 64)
    D100, I100 = ix.search(q[:B], 100)
    assert np.array_equal(I100[:, :64], I64) and np.array_equal(_bits(D100[:, :64]), _bits(D64))


def _check_range(lims, D, I, S, thr):
    hit, near = S > thr, np.abs(S - thr) <= TOL
    assert near.sum() <= NEAR_MAX * hit.sum()  # (the reference alone)
    assert lims.shape == (S.shape[0] + 1,) and lims[0] == 0 and lims[-1] == len(D) == len(I)
    for i in range(S.shape[0]):
        ids, sc = I[lims[i]:lims[i + 1]], D[lims[i]:lims[i + 1]]
        assert (np.diff(ids) > 0).all() and ids.min(initial=0) >= 0 and ids.max(initial=0) < S.shape[1], i
        assert np.abs(sc - S[i, ids]).max(initial=0) <= TOL, i
        got = np.zeros(S.shape[1], bool)
        got[ids] = True
        assert (got | near[i])[hit[i]].all() and (hit[i] | near[i])[got].all(), i  # the hit set, up to rows within TOL of the threshold


@pytest.mark.parametrize("B,thr", [(1, -1.0), (1, 0.0), (70, -1.0), (70, 0.0), (70, 0.05), (128, -1.0), (128, 0.0), (128, 0.05)])
@pytest.mark.parametrize("d", [256, 768, 1280])
def test_range(on, d, B, thr):
    q, ix, S, _ = on(d)
    _check_range(*ix.range_search(q[:B], thr), S[:B], thr)


def test_pool_regrows_under_the_batch_kernel():
    """128 x 17 000 hits are more than the initial 2^21-entry pool: the slices overflow, the counters stay exact, the scan runs again."""
    from clip_retrieval_amd.knn import build_sq8_index

    n, d, B = 17000, 256, 128
    x, q = _rows(n, d, 8), _rows(B, d, 9).astype(np.float32)
    vmin, vdiff = _ranges(x)
    ix = build_sq8_index(x, ranges=(vmin, vdiff), threshold_scan=True)
    lims, D, I = ix.range_search(q, -1.0)
    assert np.array_equal(lims, np.arange(B + 1, dtype=np.int64) * n) and np.array_equal(I.reshape(B, n), np.broadcast_to(np.arange(n), (B, n)))
    assert np.abs(D.reshape(B, n) - _reference(_encode(x, vmin, vdiff), vmin, vdiff, q, 1)[0]).max() <= TOL
    ix.close()


def test_switch_rules(tmp_path):
    from clip_retrieval_amd.knn import HipLibraryError, Mi355xIndex, build_sq8_index, load_index, save_index

    x, _, vmin, vdiff, q, _ = _corpus(256)
    ix = build_sq8_index(x[:1000], ranges=(vmin, vdiff), threshold_scan=True)
    assert ix.sq8_threshold_scan is True
    D, I = ix.search(q[:3], 100)
    assert ix.sq8_threshold_stats()[0] == 3 and ix.sq8_threshold_stats()[1] >= 1
    assert save_index(ix, str(tmp_path))["threshold_scan"] is True
    ix2 = load_index(str(tmp_path))
    assert ix2.sq8_threshold_scan is True
    D2, I2 = ix2.search(q[:3], 100)
    assert np.array_equal(I, I2) and np.array_equal(_bits(D), _bits(D2))
    ix2.sq8_threshold_scan = False  # off: the refusals of an index nobody switched on
    for call in (lambda: ix2.range_search(q[:2], 0.5), lambda: ix2.search(q[:2], 65)):
        with pytest.raises(HipLibraryError, match=r"code -5\).*flat SQ8"):
            call()
    assert "threshold_scan" not in save_index(ix2, str(tmp_path / "off"))
    empty = Mi355xIndex(256)  # not flat SQ8: the setter is an error; then flat SQ8 without a row: empty answers
    with pytest.raises(HipLibraryError, match=r"code -4\).*flat SQ8"):
        empty.sq8_threshold_scan = True
    empty.set_sq8_quantizer(vmin, vdiff)
    empty.sq8_threshold_scan = True
    assert (empty.search(q[:2], 100)[1] == -1).all() and empty.range_search(q[:2], -1.0)[0].tolist() == [0, 0, 0]
