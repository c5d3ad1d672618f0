"""The threshold scan of IVF-PQ (k > 64 and range_search behind Mi355xIndex.pq_threshold_scan) without a device: the descent state
machine driven by a stand-alone C++ program under the address and undefined-behaviour sanitizers, the numpy restatement the GPU tests
compare against (test_ivfpq_threshold_gpu.py imports it from here) with its own sanity, the rule of the saved manifest and the
threshold_scan= plumbing of the build functions."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_ivfpq_gpu import np_adc_search
from test_ivfpq_refine_cpu import _cpu_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5  # device fp32 against float64 (the bound of test_ivfpq_gpu._check)


# ------------------------------------------------------------------------------------------------ numpy restatement
def np_adc_parts(q, cent, cb, codes, lists, id_base, nprobe):
    """Per query: (ids of the rows of its probed lists, ascending; their ADC scores, float64), and the mask of queries whose probe
    set is ambiguous -- the probe rule, LUT and score of test_ivfpq_gpu.np_adc_search, every probed row kept."""
    M, _, ds = cb.shape
    nlist = cent.shape[0]
    qd = q.astype(np.float64)
    cs = qd @ cent.astype(np.float32).astype(np.float64).T
    lut = np.einsum("qmt,mjt->qmj", qd.reshape(q.shape[0], M, ds), cb.astype(np.float64))
    parts, amb = [], np.zeros(q.shape[0], dtype=bool)
    np_ = min(nprobe, nlist)
    for i in range(q.shape[0]):
        order = np.lexsort((np.arange(nlist), -cs[i]))
        if np_ < nlist and abs(cs[i, order[np_ - 1]] - cs[i, order[np_]]) <= 1e-6:
            amb[i] = True
        rows = np.flatnonzero(np.isin(lists, order[:np_]))
        S = cs[i, lists[rows]] + lut[i][np.arange(M)[None, :], codes[rows]].sum(1)
        parts.append((rows + id_base, S))
    return parts, amb


def check_range(lims, D, I, parts, amb, thr, ctx):
    """range_search against the restatement: ids ascending inside a query, every returned row a probed row whose float64 score is
    > thr - TOL, D within TOL of it, every probed row with score > thr + TOL returned.  Rows within TOL of thr may fall either way;
    there are at most max(2, 1 % of the query's hits) of them; at most 10 % of the queries are skipped for an ambiguous probe set.
    -> (largest |D - S|, largest number of rows in the band)."""
    assert lims.dtype == np.int64 and D.dtype == np.float32 and I.dtype == np.int64, ctx
    assert lims.shape == (len(parts) + 1,) and lims[0] == 0 and D.shape == I.shape == (int(lims[-1]),), ctx
    assert amb.mean() <= 0.10, f"{ctx}: {amb.mean():.2f} of the probe sets are ambiguous"
    worst, band_max = 0.0, 0
    for i, (ids, S) in enumerate(parts):
        if amb[i]:
            continue
        got, gd = I[lims[i]:lims[i + 1]], D[lims[i]:lims[i + 1]]
        assert (np.diff(got) > 0).all(), f"{ctx}: query {i}: ids not ascending (or one twice)"
        at = np.searchsorted(ids, got)
        assert (at < len(ids)).all() and np.array_equal(ids[np.minimum(at, len(ids) - 1)], got), f"{ctx}: query {i}: an id outside the probed lists"
        assert (S[at] > thr - TOL).all(), f"{ctx}: query {i}: a hit {float((thr - S[at]).max())} below the threshold"
        err = np.abs(gd.astype(np.float64) - S[at])
        worst = max(worst, float(err.max(initial=0)))
        assert err.max(initial=0) <= TOL, f"{ctx}: query {i}: score off by {err.max()}"
        sure = ids[S > thr + TOL]
        assert np.isin(sure, got).all(), f"{ctx}: query {i}: {int((~np.isin(sure, got)).sum())} rows above the threshold are missing"
        band = int((np.abs(S - thr) <= TOL).sum())
        band_max = max(band_max, band)
        assert band <= max(2, len(sure) // 100), f"{ctx}: query {i}: {band} rows within {TOL} of the threshold next to {len(sure)} hits"
    return worst, band_max


# ------------------------------------------------------------------------------------------------ the restatement's own sanity
def test_restatement_agrees_with_np_adc_search():
    x, cent, lists, cb, codes = _cpu_index(1200, 64, 12, 16, seed=3)
    rng = np.random.default_rng(0)
    q = x[rng.integers(0, len(x), 7)].astype(np.float32)
    parts, amb = np_adc_parts(q, cent, cb, codes, lists, 100, 3)
    Do, Io, amb2 = np_adc_search(q, cent, cb, codes, lists, 100, 3, 2000)
    assert np.array_equal(amb, amb2)
    for i, (ids, S) in enumerate(parts):
        assert (np.diff(ids) > 0).all()
        top = np.lexsort((ids, -S))
        assert np.array_equal(Io[i, :len(ids)], ids[top]) and (Io[i, len(ids):] == -1).all()
        assert np.array_equal(Do[i, :len(ids)], S[top])
    # a range over the restatement itself passes its own check, and a dropped sure hit does not
    thr = float(np.median(parts[0][1]))
    hits = [ids[S > thr] for ids, S in parts]
    lims = np.concatenate([[0], np.cumsum([len(h) for h in hits])]).astype(np.int64)
    I = np.concatenate(hits).astype(np.int64)
    D = np.concatenate([S[S > thr] for _, S in parts]).astype(np.float32)
    check_range(lims, D, I, parts, amb, thr, "self")
    far = int(np.argmax(parts[0][1]))  # the best row of query 0: far above the threshold
    drop = int(np.flatnonzero(hits[0] == parts[0][0][far])[0])
    lims2 = lims.copy()
    lims2[1:] -= 1
    with pytest.raises(AssertionError, match="missing"):
        check_range(lims2, np.delete(D, drop), np.delete(I, drop), parts, amb, thr, "self")


# ------------------------------------------------------------------------------------------------ the descent state machine
def _run_sanitized_check(tmp_path, name):
    """tools/<name>.cpp built with -fsanitize=address,undefined against csrc/ and run as a child process -> its standard output."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / name)
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "clip-retrieval_amd", "csrc"), os.path.join(ROOT, "tools", name + ".cpp"), "-o", exe]
    # the sanitizer runtimes linked into the program where the toolchain has them as archives (nothing then depends on the order in
    # which shared libraries are loaded); the toolchain's default otherwise
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    return run.stdout


def test_descent_state_machine_under_sanitizers(tmp_path):
    """tools/descent_check.cpp (its own main, only knnx_descent.h) built with -fsanitize=address,undefined and run as a child: the
    descent terminates within its scan budget on uniform / bell / one-close-neighbour / all-equal / T < k / T = 0 score arrays, fetches
    at least min(k, T) rows, and never fetches more than 16 k once a scan within [min(k, T), 16 k] was seen."""
    out = _run_sanitized_check(tmp_path, "descent_check")
    assert out.rstrip().endswith("descent ok") and "FAILED" not in out
    lines = [ln for ln in out.splitlines() if " scans " in ln]
    assert len(lines) >= 50
    assert any("bisections 0" not in ln for ln in lines), "no case exercised the bisection"


def test_descent_header_has_no_hip():
    text = open(os.path.join(ROOT, "clip-retrieval_amd", "csrc", "knnx_descent.h"), encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes  # system headers only, none of HIP's
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text


def test_threshold_group_driver_under_sanitizers(tmp_path):
    """tools/thr_group_check.cpp (its own main, only knnx_thr_group.h) built with -fsanitize=address,undefined and run as a child: it
    plays the device for mixed groups of queries (bell / uniform / all-equal / tied scores, totals <= 2 kc, < kc and 0, kc = 65 and
    3000, pools so small that a regrow falls among fetched queries, a full pass of 256) and asserts that every query ends fetched
    with exactly the brute-force top min(kc, total), that a fetched query only ever sees +INFINITY again, that the participations
    reported are the scans a query was not yet fetched in, and that pool_want is the smallest doubling that fits."""
    out = _run_sanitized_check(tmp_path, "thr_group_check")
    assert out.rstrip().endswith("thr group ok") and "FAILED" not in out
    lines = [ln for ln in out.splitlines() if " scans " in ln]
    assert len(lines) >= 16
    assert any(" gq 256 " in ln for ln in lines), "no group of a full pass"
    assert any("regrows 0" not in ln for ln in lines), "no case made the pool grow"
    assert any("mixed steps 0" not in ln for ln in lines), "no step had a final query next to a descending one"


def test_threshold_group_header_has_no_hip():
    text = open(os.path.join(ROOT, "clip-retrieval_amd", "csrc", "knnx_thr_group.h"), encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    # system headers and the descent (itself checked above), none of HIP's
    assert includes and all((inc.startswith("<") and "hip" not in inc) or inc == '"knnx_descent.h"' for inc in includes), includes
    assert '"knnx_descent.h"' in includes
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text


# ------------------------------------------------------------------------------------------------ manifest and plumbing
def test_manifest_flag_rules():
    from clip_retrieval_amd import knn

    assert knn.ivfpq_threshold_scan_entry(False) == {} and knn.ivfpq_threshold_scan_entry(True) == {"threshold_scan": True}
    assert knn.read_ivfpq_threshold_scan("f", {"format": knn.IVFPQ_FORMAT}) is False  # every folder written before the switch existed
    assert knn.read_ivfpq_threshold_scan("f", {"threshold_scan": True}) is True
    assert knn.read_ivfpq_threshold_scan("f", {"threshold_scan": False}) is False
    for bad in (1, "true", None, [True]):
        with pytest.raises(ValueError, match="threshold_scan"):
            knn.read_ivfpq_threshold_scan("f", {"threshold_scan": bad})


class _StubLib:
    """Just enough of the library for _ivfpq_begin: records the calls, answers KNNX_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("knnx_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0

        return call


def _begin_with_stub(monkeypatch, **kw):
    from clip_retrieval_amd import knn, knn_build

    lib = _StubLib()

    class StubIndex:
        def __init__(self, d, device=0, id_base=0):
            self.d, self._dpad, self._lib, self._h = d, d, lib, 1

        def set_pq_quantizer(self, M, cb):
            lib.calls.append(("set_pq_quantizer", (M,)))

        def _pad(self, a):
            return a

        k_factor = 1
        pq_threshold_scan = knn.Mi355xIndex.pq_threshold_scan

    monkeypatch.setattr(knn_build, "Mi355xIndex", StubIndex)  # (where _ivfpq_begin looks the class up)
    cent = np.zeros((4, 64), np.float16)
    knn._ivfpq_begin(64, 4, 16, cent, np.zeros((16, 256, 4), np.float32), np.ones(4, np.int64), 0, 0, **kw)  # pylint: disable=protected-access
    return [c for c in lib.calls if c[0] == "knnx_ivfpq_set_threshold_scan"], [c[0] for c in lib.calls]


def test_ivfpq_begin_passes_the_switch(monkeypatch):
    on, names = _begin_with_stub(monkeypatch, threshold_scan=True)
    assert len(on) == 1 and on[0][1][1] == 1
    assert names.index("knnx_ivfpq_set_threshold_scan") < names.index("knnx_ivf_begin")
    off, _ = _begin_with_stub(monkeypatch, threshold_scan=False)
    assert off == []  # off is the state of a new index: a default build makes exactly the calls it always made
    default, _ = _begin_with_stub(monkeypatch)
    assert default == []


def test_build_functions_take_threshold_scan():
    import inspect

    from clip_retrieval_amd import knn

    for fn in (knn.build_ivfpq_index, knn.build_ivfpq_index_from_folder, knn.build_ivfpq_index_device, knn._ivfpq_begin):  # pylint: disable=protected-access
        p = inspect.signature(fn).parameters
        assert "threshold_scan" in p and p["threshold_scan"].default is False, fn.__name__
    for cls in (knn.Mi355xIndex, knn.ShardedMi355xIndex):
        prop = cls.pq_threshold_scan
        assert isinstance(prop, property) and prop.fset is not None, cls.__name__
