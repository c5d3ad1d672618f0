"""The device post filter (knnx_search_filtered) without a GPU: the integer arithmetic of csrc/knnx_filter_plan.h driven by a stand-alone
program under the sanitizers, the header's freedom from HIP, the three exported symbols and their refusals on null arguments and
k = 8193, and the request assembly of `KnnHotPath(device_filter=True)` over a stub index against the general path on the same rows."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clip-retrieval_amd", "csrc")


def test_filter_plan_under_sanitizers(tmp_path):
    """tools/filter_plan_check.cpp (its own main, only knnx_filter_plan.h) built with -fsanitize=address,undefined and run as a child:
    every tile of the upper triangle is visited exactly once for nt = 1 .. 130, the scratch sizes, and the hook / compress rounds end at
    the union-find answer within their bound on paths, stars, cliques, two components joined by their largest members and random
    graphs, under shuffled link orders."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "filter_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            os.path.join(ROOT, "tools", "filter_plan_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked into the program where the toolchain has them as archives; the toolchain's default otherwise
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("filter plan ok") and "FAILED" not in run.stdout
    assert "nt = 1 .. 130" in run.stdout
    for shape in ("path in scrambled ranks", "star around the largest", "clique", "two paths joined at their largest", "random"):
        assert shape in run.stdout, shape


def test_header_has_no_hip():
    text = open(os.path.join(CSRC, "knnx_filter_plan.h"), encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all("hip" not in inc for inc in includes), includes
    assert all(inc.startswith("<") for inc in includes), includes  # system headers only
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text and "hipError" not in text


def test_sources_are_in_the_makefile():
    mk = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS = (.*)$", mk, re.M).group(1).split()
    assert "knn_filter_kernels.hip" in srcs and "knnx_filter.hip" in srcs and "knnx_filter_plan.h" in hdrs


def test_symbols_are_declared_and_exported(lib):
    from clip_retrieval_amd._lib import SIGNATURES

    header = open(os.path.join(ROOT, "include", "knnx.h"), encoding="utf-8").read()
    for name in ("knnx_search_filtered", "knnx_mlp_forward_device", "knnx_mlp_device"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib, name) and name in SIGNATURES, name
    for macro, value in (("KNNX_FILTER_MAX_K", 8192), ("KNNX_DROP_DUPLICATE", 1), ("KNNX_DROP_VIOLENT", 2), ("KNNX_DROP_UNSAFE", 4)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", header), macro
    assert re.search(r"int32_t n_valid, n_links, links_overflowed, cc_rounds;\s*}\s*knnx_filter_stats;", header)


def test_refusals_are_visible_without_a_device(lib):
    q = np.zeros(256, np.float32)
    D, I, drop = np.zeros(8193, np.float32), np.zeros(8193, np.int64), np.zeros(8193, np.uint8)
    # k above the limit is refused before anything else is looked at, with the limit in the message
    rc = lib.knnx_search_filtered(None, q.ctypes.data, 8193, 256, 1, C.c_float(0.94), None, None, C.c_float(0.5), D.ctypes.data,
                                  I.ctypes.data, drop.ctypes.data, None)
    assert rc == -5 and b"8192" in lib.knnx_last_error()
    # null index / query / outputs
    rc = lib.knnx_search_filtered(None, q.ctypes.data, 40, 256, 1, C.c_float(0.94), None, None, C.c_float(0.5), D.ctypes.data,
                                  I.ctypes.data, drop.ctypes.data, None)
    assert rc == -1 and b"search_filtered" in lib.knnx_last_error()
    assert lib.knnx_mlp_device(None) == -1
    y = np.zeros(4, np.float32)
    assert lib.knnx_mlp_forward_device(None, q.ctypes.data, 256, 1, y.ctypes.data, None) == -1
    assert b"mlp_forward_device" in lib.knnx_last_error()


# ---- the request assembly behind the drop bytes ----------------------------------------------------------------------------------
def _non_uniques_numpy(emb, thr=0.94):
    emb = np.asarray(emb, dtype=np.float64)
    n = emb.shape[0]
    sim = emb @ emb.T
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j in zip(*np.nonzero(np.triu(sim > thr, 1))):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return [i for i in range(n) if find(i) != i]


class _StubHead:
    """Stands for a resident head: numpy scores, a device number."""

    def __init__(self, w, device=0):
        self.w, self.device, self.calls = np.asarray(w, np.float32), device, 0

    def predict(self, x, batch_size=None):  # pylint: disable=unused-argument
        self.calls += 1
        return np.asarray(x, np.float32) @ self.w.T


def _canned(seed, k, d=32):
    """Rows with near-duplicate groups, ids with repeats and a -1 tail."""
    rng = np.random.default_rng(seed)
    n = k - 7
    rows = rng.standard_normal((n, d)).astype(np.float32)
    for src, dst in ((3, 9), (9, 20), (50, 4), (60, 61), (61, 62)):  # chains: 3-9-20 and 50-4, 60-61-62
        rows[dst] = rows[src] + 0.01 * rng.standard_normal(d).astype(np.float32)
    ids = rng.permutation(10 * n)[:n].astype(np.int64)
    ids[30] = ids[5]    # the same id twice: reported once, at its best rank
    ids[70] = ids[9]    # a repeat of an id the filter drops
    rows[30], rows[70] = rows[5], rows[9]
    I = np.full((1, k), -1, np.int64)
    I[0, :n] = ids
    D = np.sort(rng.random((1, k)).astype(np.float32))[:, ::-1].copy()
    return D, I, rows


class _StubIndex:
    device = 0

    def __init__(self, D, I, rows, bits, overflow=False):
        self.D, self.I, self.rows, self.bits, self.overflow = D, I, rows, bits, overflow
        self.filtered_calls = self.general_calls = self.reconstructs = 0
        self.by_id = {}
        for i, r in zip(I[0], rows):
            self.by_id[int(i)] = r

    def search_filtered(self, x, k, dedup_thr=None, violence=None, safety=None, safety_thr=0.5):  # pylint: disable=unused-argument
        self.filtered_calls += 1
        self.last = dict(k=k, dedup_thr=dedup_thr, violence=violence, safety=safety, safety_thr=safety_thr)
        bits = self.bits.copy()
        if dedup_thr is None or self.overflow:
            bits &= ~np.uint8(1)
        if violence is None:
            bits &= ~np.uint8(2)
        if safety is None:
            bits &= ~np.uint8(4)
        n = self.rows.shape[0]
        return self.D.copy(), self.I.copy(), bits, dict(n_valid=n, n_links=(1 << 20) + 5 if self.overflow else 7,
                                                        links_overflowed=int(self.overflow), cc_rounds=0 if self.overflow else 3)

    def search_and_reconstruct(self, x, k):  # pylint: disable=unused-argument
        self.general_calls += 1
        R = np.zeros((1, k, self.rows.shape[1]), np.float32)
        R[0, : self.rows.shape[0]] = self.rows
        return self.D.copy(), self.I.copy(), R

    def search(self, x, k):  # pylint: disable=unused-argument
        self.general_calls += 1
        return self.D.copy(), self.I.copy()

    def reconstruct_batch(self, keys):
        self.reconstructs += 1
        return np.stack([self.by_id[int(i)] for i in keys]).astype(np.float32)


@pytest.mark.parametrize("overflow", [False, True])
@pytest.mark.parametrize("filters", [(True, False, False), (True, True, True), (False, True, True), (False, False, True)])
def test_hot_path_assembly_over_a_stub_index(monkeypatch, filters, overflow):
    """KnnHotPath(device_filter=True) over a stub index whose search_filtered returns canned (D, I, drop) gives the lists the general
    path gives on the same canned rows: repeated ids, a -1 tail, an id the filter drops occurring twice, and the overflow flag (dedup
    alone re-run through reconstruct_batch + get_non_uniques).  With the switch off the stub's method is never called."""
    from types import SimpleNamespace

    from clip_retrieval_amd.service import KnnHotPath, Mi355xSafetyHead, normalized

    dedup, use_violence, use_safety = filters
    k, d = 100, 32
    D, I, rows = _canned(7, k, d)
    emb = normalized(rows)
    rng = np.random.default_rng(11)
    prompts = rng.standard_normal((2, d)).astype(np.float32)
    safety_w = rng.standard_normal((1, d)).astype(np.float32) * 3
    bits = np.zeros(k, np.uint8)
    bits[_non_uniques_numpy(emb)] |= 1
    bits[: len(emb)][np.argmax(emb @ prompts.T, axis=1) == 1] |= 2
    bits[: len(emb)][(emb @ safety_w.T)[:, 0] > 0.5] |= 4
    assert np.count_nonzero(bits & 1) == 7 and 0 < np.count_nonzero(bits & 2) < len(emb) and 0 < np.count_nonzero(bits & 4) < len(emb)

    # a safety head that passes for a device head without a device, and the prompt head of the violence detector likewise
    safety = object.__new__(Mi355xSafetyHead)
    stub = _StubHead(safety_w)
    safety.device, safety.predict, safety._h = 0, stub.predict, None  # pylint: disable=protected-access
    prompt_head = _StubHead(prompts)
    monkeypatch.setattr(KnnHotPath, "_prompt_head", lambda self, p: prompt_head)
    monkeypatch.setattr(KnnHotPath, "get_non_uniques", lambda self, e, threshold=0.94: _non_uniques_numpy(e, threshold))

    for mapped in (False, True):
        table = np.arange(10 * k, dtype=np.int64)[::-1].copy()
        answers = []
        for on in (False, True):
            index = _StubIndex(D, I, rows, bits, overflow)
            res = SimpleNamespace(image_index=index, text_index=index, safety_model=safety, violence_detector=prompts,
                                  metadata_is_ordered_by_ivf=mapped, ivf_old_to_new_mapping=table if mapped else None)
            hot = KnnHotPath(device_filter=on)
            answers.append(hot.knn_search(np.zeros((1, d), np.float32), "image", k, res, dedup, use_safety, use_violence))
            if on:
                assert index.filtered_calls == 1 and index.general_calls == 0
                assert index.last["k"] == k and (index.last["dedup_thr"] == 0.94) == dedup
                assert (index.last["violence"] is prompt_head) == use_violence and (index.last["safety"] is safety) == use_safety
                assert index.reconstructs == (1 if overflow and dedup else 0)
            else:
                assert index.filtered_calls == 0 and index.general_calls == 1
        (d_off, i_off), (d_on, i_on) = answers
        assert [int(i) for i in i_on] == [int(i) for i in i_off] and [float(x) for x in d_on] == [float(x) for x in d_off]
        assert len(i_on) == len(set(int(i) for i in i_on)) and -1 not in i_on and 0 < len(i_on) < k - 7


def test_hot_path_keeps_the_general_path_where_the_device_filter_does_not_apply(monkeypatch):
    """Switch on, but: k <= 64 without a safety / violence filter, k > 8192, an index without search_filtered, a safety model that is
    not a device head, a head on another device -- the stub's search_filtered is never called."""
    from types import SimpleNamespace

    from clip_retrieval_amd.service import KnnHotPath, Mi355xSafetyHead

    d = 32
    monkeypatch.setattr(KnnHotPath, "get_non_uniques", lambda self, e, threshold=0.94: _non_uniques_numpy(e, threshold))
    D, I, rows = _canned(3, 100, d)
    w = np.ones((1, d), np.float32)
    other = object.__new__(Mi355xSafetyHead)
    other.device, other.predict, other._h = 1, _StubHead(w).predict, None  # pylint: disable=protected-access
    cases = [
        dict(k=100, safety=_StubHead(w), use_safety=True),   # any other type with .predict: the general path
        dict(k=100, safety=other, use_safety=True),          # a device head, but on device 1
    ]
    for c in cases:
        index = _StubIndex(D, I, rows, np.zeros(100, np.uint8))
        res = SimpleNamespace(image_index=index, text_index=index, safety_model=c["safety"], violence_detector=None)
        KnnHotPath(device_filter=True).knn_search(np.zeros((1, d), np.float32), "image", c["k"], res, True, c["use_safety"], False)
        assert index.filtered_calls == 0 and index.general_calls == 1, c
    # k <= 64 and dedup alone: not this path's (a stub without search_dedup takes search_and_reconstruct)
    index = _StubIndex(D[:, :40].copy(), I[:, :40].copy(), rows[:40], np.zeros(40, np.uint8))
    res = SimpleNamespace(image_index=index, text_index=index, safety_model=None, violence_detector=None)
    KnnHotPath(device_filter=True).knn_search(np.zeros((1, d), np.float32), "image", 40, res, True, True, True)
    assert index.filtered_calls == 0 and index.general_calls == 1
    # no filter at all, any k
    index = _StubIndex(D, I, rows, np.zeros(100, np.uint8))
    res = SimpleNamespace(image_index=index, text_index=index, safety_model=None, violence_detector=None)
    KnnHotPath(device_filter=True).knn_search(np.zeros((1, d), np.float32), "image", 100, res, False, False, False)
    assert index.filtered_calls == 0 and index.general_calls == 1
    # k above the device filter's limit
    k = 8200
    Dk, Ik, rowsk = _canned(5, k, d)
    index = _StubIndex(Dk, Ik, rowsk[:200], np.zeros(k, np.uint8))
    index.I[0, 200:] = -1
    res = SimpleNamespace(image_index=index, text_index=index, safety_model=None, violence_detector=None)
    KnnHotPath(device_filter=True).knn_search(np.zeros((1, d), np.float32), "image", k, res, True, False, False)
    assert index.filtered_calls == 0 and index.general_calls == 1
    # an index without the method (the sharded index)
    index = _StubIndex(D, I, rows, np.zeros(100, np.uint8))
    bare = SimpleNamespace(search_and_reconstruct=index.search_and_reconstruct, search=index.search, device=0)
    res = SimpleNamespace(image_index=bare, text_index=bare, safety_model=None, violence_detector=None)
    KnnHotPath(device_filter=True).knn_search(np.zeros((1, d), np.float32), "image", 100, res, True, False, False)
    assert index.filtered_calls == 0 and index.general_calls == 1
