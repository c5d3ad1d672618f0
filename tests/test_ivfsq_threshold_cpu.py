"""The threshold scan of IVF-SQ8 (k > 64 and range_search behind Mi355xIndex.sq_threshold_scan) without a device: the rule of the saved
manifest, the threshold_scan= plumbing of the build functions, and the numpy statement the GPU tests rest on -- the range hits of a
query are a prefix of its full ranking."""
import inspect
import json

import numpy as np
import pytest

from test_ivfsq_cpu import corpus, np_ranges, np_sq_encode, np_sq_scores, np_sq_search


def test_manifest_flag_rules(tmp_path):
    """{"threshold_scan": true} only when the switch is on; a folder without the key reads as off; a non-boolean is an error; the
    manifest function and its check keep their results."""
    from clip_retrieval_amd import knn

    assert knn.ivfsq_threshold_scan_entry(True) == {"threshold_scan": True}
    assert knn.ivfsq_threshold_scan_entry(False) == {} and knn.ivfsq_threshold_scan_entry(0) == {}
    man = knn.ivfsq_manifest(768, 4096, 16, (1000, 7000))
    assert "threshold_scan" not in man
    assert man == {"format": knn.IVFSQ_FORMAT, "kind": "ivfsq", "d": 768, "nlist": 4096, "nprobe": 16, "row_range": [1000, 7000]}
    assert knn.read_ivfsq_threshold_scan("x", man) is False
    on = {**man, **knn.ivfsq_threshold_scan_entry(True)}
    p = tmp_path / knn.IVFSQ_MANIFEST
    p.write_text(json.dumps(on), encoding="utf-8")
    back = knn.check_ivfsq_manifest(json.loads(p.read_text(encoding="utf-8")), str(p))
    assert back == on and knn.read_ivfsq_threshold_scan(str(p), back) is True
    assert knn.read_ivfsq_threshold_scan("x", {**man, "threshold_scan": False}) is False
    for bad in (1, 0, "true", None, [True]):
        with pytest.raises(ValueError, match="threshold_scan"):
            knn.read_ivfsq_threshold_scan("x", {**man, "threshold_scan": bad})


def test_build_functions_take_threshold_scan():
    from clip_retrieval_amd import knn

    for fn in (knn.build_ivfsq_index, knn.build_ivfsq_index_from_folder, knn.build_ivfsq_index_device):
        p = inspect.signature(fn).parameters
        assert "threshold_scan" in p and p["threshold_scan"].default is False, fn.__name__
    for fn in (knn._ivfsq_begin, knn._ivfsq_encode_chunks, knn._ivfsq_from_codes):  # pylint: disable=protected-access
        assert inspect.signature(fn).parameters["threshold_scan"].default is False, fn.__name__
    for cls in (knn.Mi355xIndex, knn.ShardedMi355xIndex):
        prop = cls.sq_threshold_scan
        assert isinstance(prop, property) and prop.fset is not None
    assert callable(knn.Mi355xIndex.sq_threshold_stats)


def test_ivfsq_begin_passes_the_switch(monkeypatch):
    """_ivfsq_begin switches a new index on when asked and calls nothing for it otherwise."""
    from clip_retrieval_amd import knn, knn_build

    calls = []

    class Fake:
        _h = 1

        def __init__(self, d, device=0, id_base=0):
            self._lib = type("L", (), {"knnx_ivf_begin": staticmethod(lambda *a: 0)})()

        def set_sq_quantizer(self, vmin, vdiff):
            pass

        def _pad(self, a):
            return a

        sq_threshold_scan = property(lambda self: False, lambda self, v: calls.append(v))

    monkeypatch.setattr(knn_build, "Mi355xIndex", Fake)  # (where _ivfsq_begin and _ivf_begin look the names up)
    monkeypatch.setattr(knn_build, "check", lambda lib, rc, which: None)
    cent, sizes = np.zeros((2, 256), np.float16), np.array([1, 2])
    knn._ivfsq_begin(256, 2, cent, (np.zeros(256), np.zeros(256)), sizes, 0, 0)  # pylint: disable=protected-access
    assert calls == []
    knn._ivfsq_begin(256, 2, cent, (np.zeros(256), np.zeros(256)), sizes, 0, 0, True)  # pylint: disable=protected-access
    assert calls == [True]


@pytest.mark.parametrize("nprobe", [1, 3, 8])
def test_range_hits_are_a_prefix_of_the_full_ranking(nprobe):
    """The rows of the probed lists with score > thresh are the first rows of the k = N + 10 ranking: what lets a large-k search take the
    top k of a threshold scan's hits, and what the GPU test's range reference (np_sq_search filtered by > thresh) relies on."""
    n, d, nlist = 700, 256, 8
    x = corpus("mixture", d, n)
    rng = np.random.default_rng(3)
    lists = rng.integers(0, nlist, n).astype(np.int32)
    cent = np.stack([x[lists == l].astype(np.float32).mean(0) for l in range(nlist)])
    cent = (cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(np.float16)
    vmin, vdiff = np_ranges(x)
    codes = np_sq_encode(x, vmin, vdiff)
    q = x[rng.integers(0, n, 9)].astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    D, I, _ = np_sq_search(q, cent, codes, lists, vmin, vdiff, 0, nprobe, n + 10)
    S = np_sq_scores(q, codes, vmin, vdiff)
    cs = q.astype(np.float64) @ cent.astype(np.float32).astype(np.float64).T
    for i in range(9):
        probed = np.lexsort((np.arange(nlist), -cs[i]))[:nprobe]
        rows = np.flatnonzero(np.isin(lists, probed))
        valid = I[i] >= 0
        assert valid.sum() == len(rows) and not valid[len(rows):].any()  # every probed row, then padding
        for thr in (-1.0, 0.0, 0.3, float(np.median(S[i, rows]))):
            want = rows[S[i, rows] > thr]  # ascending ids
            m = len(want)
            assert np.array_equal(np.sort(I[i, :m]), want)
            assert (D[i, :m] > thr).all() and (m == len(rows) or D[i, m] <= thr)
