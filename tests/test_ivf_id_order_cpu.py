"""List-ordered ids (reorder_metadata_by_ivf_index) without a GPU: the host arithmetic of csrc/knnx_id_order.h driven by a stand-alone
program under the sanitizers, the header's freedom from HIP, the loud failure of the new entry points, KnnHotPath.knn_search with
metadata_is_ordered_by_ivf over fake index objects, the raw mapping file of the reference and the Arrow re-ordering."""
import ctypes as C
import os
import shutil
import subprocess
import threading
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ numpy restatement
def np_id_order(list_ids, id_base=0):
    """list_ids: one array of ids per inverted list, in arena order -> (old_to_new, new_to_old) as include/knnx.h defines them
    (ivf_metadata_ordering.py:46-64 with np.put)."""
    new_to_old = np.concatenate([np.asarray(a, dtype=np.int64) for a in list_ids]) if list_ids else np.zeros(0, np.int64)
    old_to_new = np.ones(new_to_old.shape[0], dtype=np.int64)
    old_to_new.put(new_to_old - id_base, np.arange(new_to_old.shape[0], dtype=np.int64) + id_base)
    return old_to_new, new_to_old


def np_map_ids(old_to_new, ids, id_base=0):
    ids = np.asarray(ids, dtype=np.int64)
    return np.where(ids == -1, -1, np.take(old_to_new, np.where(ids == -1, 0, ids - id_base)))


# ------------------------------------------------------------------------------------------------ the header
def test_host_arithmetic_under_sanitizers(tmp_path):
    """tools/id_order_check.cpp (its own main, only knnx_id_order.h) built with -fsanitize=address,undefined and run as a child:
    dense0 with empty lists at the front, in a run in the middle and at the end; chunk plans for ntotal in {1, 63, 64, 65, 162} at
    chunk 64 covering every ordinal once; the range check below id_base, at id_base + ntotal and for -1; shard routing with 1, 2 and
    3 shards, both sides of every boundary, duplicates, -1 and an id past the last shard."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "id_order_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "clip-retrieval_amd", "csrc"), os.path.join(ROOT, "tools", "id_order_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked into the program where the toolchain has them as archives; the toolchain's default otherwise
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert run.stdout.rstrip().endswith("id order ok") and "FAILED" not in run.stdout
    assert sum(ln.startswith("dense0 ") for ln in lines) >= 8
    for total in (1, 63, 64, 65, 162):
        assert any(ln.startswith(f"chunks total {total:4d} chunk  64") for ln in lines), total
    assert sum(ln.startswith("range ") for ln in lines) >= 8
    assert sum(ln.startswith("route ") for ln in lines) >= 8
    for shards in (1, 2, 3):
        assert any(ln.startswith("route ") and f"shards {shards} " in ln for ln in lines), shards


def test_header_has_no_hip():
    text = open(os.path.join(ROOT, "clip-retrieval_amd", "csrc", "knnx_id_order.h"), encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes  # system headers only, none of HIP's
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text and "hipError" not in text


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_new_entry_points_fail_loudly(lib):
    """Null handles answer KNNX_E_ARG with a message; with no GPU an index cannot even be created, so nothing falls back to the CPU."""
    import torch

    from clip_retrieval_amd import HipLibraryError

    buf = (C.c_int64 * 4)(0, 1, 2, 3)
    for name, args in (("knnx_ivf_id_order", (None, buf, buf)), ("knnx_ivf_map_ids", (None, buf, 4, buf)),
                       ("knnx_shards_id_order", (None, buf, buf)), ("knnx_shards_map_ids", (None, buf, 4, buf))):
        assert getattr(lib, name)(*args) == -1, name  # KNNX_E_ARG
        assert b"null" in lib.knnx_last_error(), name
    assert list(buf) == [0, 1, 2, 3]
    if not torch.cuda.is_available():
        from clip_retrieval_amd.knn import Mi355xIndex

        with pytest.raises(HipLibraryError):
            Mi355xIndex(256)


def test_package_exports_the_reference_names():
    import clip_retrieval_amd
    from clip_retrieval_amd import knn, service

    assert clip_retrieval_amd.get_old_to_new_mapping is knn.get_old_to_new_mapping
    assert clip_retrieval_amd.search_to_new_ids is knn.search_to_new_ids
    assert clip_retrieval_amd.load_ivf_old_to_new_mapping is service.load_ivf_old_to_new_mapping
    assert clip_retrieval_amd.reorder_arrow_metadata is service.reorder_arrow_metadata
    with pytest.raises(AttributeError):
        clip_retrieval_amd.no_such_name  # pylint: disable=pointless-statement


# ------------------------------------------------------------------------------------------------ KnnHotPath over fake indexes
class FakeIndex:
    """Pure-Python stand-in with the faiss-shaped surface knn_search calls, and map_ids over its own permutation."""
    d = 8

    def __init__(self, D, I, seed, links=None):
        rng = np.random.default_rng(seed)
        self.D, self.I, self.links = D, I, links
        self.R = rng.standard_normal((1, I.shape[1], 8)).astype(np.float32)
        self.perm = rng.permutation(1000).astype(np.int64)  # old_to_new of THIS index
        self.mapped = []  # every array handed to map_ids

    def search(self, q, k):
        return self.D.copy(), self.I.copy()

    def search_and_reconstruct(self, q, k):
        return self.D.copy(), self.I.copy(), self.R.copy()

    def search_dedup(self, q, k, thr, want_r=False):
        return self.D.copy(), self.I.copy(), (self.R.copy() if want_r else None), self.links.copy()

    def map_ids(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        self.mapped.append(ids.copy())
        assert (ids >= 0).all(), "-1 reached the mapping"
        return self.perm[ids]


class Safety:  # flags result rank 1
    def predict(self, emb, batch_size=None):
        y = np.zeros((emb.shape[0], 1), np.float32)
        y[1] = 1.0
        return y


def _hot_path():
    from clip_retrieval_amd.service import KnnHotPath

    hp = KnnHotPath.__new__(KnnHotPath)  # (no GPU: the dedup pool and the prompt cache are not touched by these requests)
    hp._nprobe_lock = threading.Lock()  # pylint: disable=protected-access
    return hp


K = 12
CASES = {
    "distinct": np.arange(100, 100 + K, dtype=np.int64)[None],
    "short": np.r_[np.arange(5, 12), -np.ones(5)].astype(np.int64)[None],
    "repeated ids": np.asarray([[4, 9, 4, 7, 9, 1, 2, 3, 5, 6, 8, 4]], dtype=np.int64),
}
LINKS = (np.zeros((0, 2), np.int32), np.asarray([[0, 3], [3, 6], [2, 5]], np.int32))


@pytest.mark.parametrize("modality", ["image", "text"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_knn_search_with_metadata_ordered_by_ivf(case, modality):
    """metadata_is_ordered_by_ivf=True gives the survivors of the same request with False, translated -- through the IMAGE index's
    mapping for both modalities, after the cut at -1 and the filters, on the fast return path too; an explicit
    ivf_old_to_new_mapping array wins over map_ids.  (On the parent commit: NotImplementedError.)"""
    hp = _hot_path()
    rng = np.random.default_rng(7)
    D = np.sort(rng.random((1, K)).astype(np.float32))[:, ::-1].copy()
    I = CASES[case]
    q = np.zeros((1, 8), np.float32)
    n_valid = int(np.argmax(I[0] == -1)) if (I[0] == -1).any() else K
    for links in LINKS:
        for dedup, safety in ((False, False), (True, False), (True, True), (False, True)):
            image, text = FakeIndex(D, I, 1, links), FakeIndex(D, I, 2, links)
            assert not np.array_equal(image.perm, text.perm)
            res = SimpleNamespace(image_index=image, text_index=text, metadata_is_ordered_by_ivf=False, ivf_old_to_new_mapping=None,
                                  safety_model=Safety() if safety else None, violence_detector=None)
            d0, i0 = hp.knn_search(q, modality, K, res, dedup, safety, False)
            assert not image.mapped and not text.mapped, "False must not translate anything"
            res.metadata_is_ordered_by_ivf = True
            d1, i1 = hp.knn_search(q, modality, K, res, dedup, safety, False)
            ctx = (case, modality, len(links), dedup, safety)
            assert np.array_equal(np.asarray(d1), np.asarray(d0)), ctx
            assert [int(v) for v in i1] == [int(image.perm[int(v)]) for v in i0], ctx  # the image index's mapping, whichever was searched
            assert not text.mapped, ctx
            assert len(image.mapped) == 1 and image.mapped[0].tolist() == [int(v) for v in i0], ctx  # survivors only: the fewest ids travel
            assert len(i0) <= n_valid and all(hasattr(v, "item") for v in i1), ctx
            if not dedup and not safety and case != "repeated ids":
                assert len(i1) == n_valid, ctx  # the fast return path (nothing to drop, every id once) translates as well
            # the reference's array wins over map_ids and works with any index object
            table = np.random.default_rng(3).permutation(1000).astype(np.int64)
            res.ivf_old_to_new_mapping = table
            image.mapped.clear()
            d2, i2 = hp.knn_search(q, modality, K, res, dedup, safety, False)
            assert not image.mapped and not text.mapped, ctx
            assert [int(v) for v in i2] == [int(table[int(v)]) for v in i0] and np.array_equal(np.asarray(d2), np.asarray(d0)), ctx


def test_knn_search_maps_nothing_when_everything_is_cut():
    hp = _hot_path()
    I = -np.ones((1, K), dtype=np.int64)
    D = np.full((1, K), -3.4028234663852886e38, dtype=np.float32)
    image = FakeIndex(D, I, 1, LINKS[0])
    res = SimpleNamespace(image_index=image, text_index=image, metadata_is_ordered_by_ivf=True, ivf_old_to_new_mapping=None,
                          safety_model=None, violence_detector=None)
    d, i = hp.knn_search(np.zeros((1, 8), np.float32), "image", K, res, False, False, False)
    assert d == [] and i == []
    assert all(m.size == 0 for m in image.mapped)


# ------------------------------------------------------------------------------------------------ the mapping file
class _MappingIndex:
    def __init__(self, mapping):
        self.mapping, self.calls = mapping, 0

    def ivf_old_to_new(self):
        self.calls += 1
        return self.mapping.copy()


def test_mapping_file_is_the_reference_s_raw_memmap(tmp_path):
    """clip_back.py:629-640: `ivf_old_to_new_mapping.npy` is a raw int64 memmap with no npy header, written once when absent and
    mapped read-only afterwards; a file written by the reference's three lines loads, and ours loads with the reference's line."""
    from clip_retrieval_amd.service import IVF_MAPPING_FILE, load_ivf_old_to_new_mapping

    assert IVF_MAPPING_FILE == "ivf_old_to_new_mapping.npy"
    mapping = np.random.default_rng(0).permutation(5000).astype(np.int64)
    ours = tmp_path / "ours"
    ours.mkdir()
    ix = _MappingIndex(mapping)
    got = load_ivf_old_to_new_mapping(str(ours), ix)
    path = ours / IVF_MAPPING_FILE
    assert isinstance(got, np.memmap) and got.dtype == np.int64 and not got.flags.writeable and np.array_equal(got, mapping)
    assert path.stat().st_size == mapping.size * 8 and path.read_bytes() == mapping.tobytes()  # raw: no header
    assert os.listdir(ours) == [IVF_MAPPING_FILE]
    again = load_ivf_old_to_new_mapping(str(ours), ix)
    assert ix.calls == 1 and np.array_equal(again, mapping), "the file is written once"
    assert np.array_equal(np.memmap(str(path), dtype="int64", mode="r"), mapping)  # the reference's reading line
    # the reference's writing lines, restated
    theirs = tmp_path / "theirs"
    theirs.mkdir()
    other = np.random.default_rng(1).permutation(777).astype(np.int64)
    w = np.memmap(str(theirs / IVF_MAPPING_FILE), dtype="int64", mode="write", shape=other.shape)
    w[:] = other
    del w
    never = _MappingIndex(mapping)
    got = load_ivf_old_to_new_mapping(str(theirs), never)
    assert never.calls == 0 and got.shape == (777,) and np.array_equal(got, other)


# ------------------------------------------------------------------------------------------------ Arrow re-ordering
def write_arrow_folder(folder, n, files, seed=0):
    """n rows over `files` Arrow IPC files (two record batches each): a string column, an int column and a float column."""
    pa = pytest.importorskip("pyarrow")
    rng = np.random.default_rng(seed)
    os.makedirs(folder, exist_ok=True)
    url = [f"http://x/{i}-{'y' * int(rng.integers(0, 9))}" for i in range(n)]
    table = pa.table({"url": url, "row": np.arange(n, dtype=np.int64), "score": rng.random(n).astype(np.float32)})
    cuts = np.linspace(0, n, files + 1).astype(int)
    for f in range(files):
        part = table.slice(cuts[f], cuts[f + 1] - cuts[f])
        with pa.OSFile(os.path.join(folder, f"{f}.arrow"), "wb") as sink, pa.ipc.new_file(sink, table.schema) as writer:
            for batch in part.to_batches(max_chunksize=max(1, (cuts[f + 1] - cuts[f] + 1) // 2)):
                writer.write_batch(batch)
    return table


class _PermIndex:
    def __init__(self, new_to_old):
        self.n2o = np.asarray(new_to_old, dtype=np.int64)
        self.o2n = np.empty_like(self.n2o)
        self.o2n[self.n2o] = np.arange(self.n2o.size)

    def ivf_new_to_old(self):
        return self.n2o.copy()

    def map_ids(self, ids):
        return self.o2n[np.asarray(ids, dtype=np.int64)]


def test_reorder_arrow_metadata_against_a_numpy_permutation(tmp_path):
    """500 rows in 3 Arrow files with a string column, rows_per_file = 128: row o of the result is source row new_to_old[o], so the
    re-ordered provider asked for map_ids(ids) answers exactly what the original answers for ids."""
    pytest.importorskip("pyarrow")
    from clip_retrieval_amd.service import ArrowMetadataProvider, reorder_arrow_metadata

    n = 500
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    table = write_arrow_folder(src, n, 3)
    ix = _PermIndex(np.random.default_rng(5).permutation(n))
    written = reorder_arrow_metadata(ix, src, dst, rows_per_file=128)
    assert [os.path.basename(p) for p in written] == ["00000.arrow", "00001.arrow", "00002.arrow", "00003.arrow"]
    assert sorted(os.listdir(dst)) == [os.path.basename(p) for p in written]
    old, new = ArrowMetadataProvider(src), ArrowMetadataProvider(dst)
    assert new.table.num_rows == n and new.table.schema.names == ["url", "row", "score"]
    assert new.table.column("row").to_numpy().tolist() == ix.n2o.tolist()  # row o = source row new_to_old[o]
    assert new.table.column("url").to_pylist() == [table.column("url")[int(i)].as_py() for i in ix.n2o]
    ids = np.r_[np.random.default_rng(6).integers(0, n, 60), 0, n - 1, 127, 128, 7, 7]
    assert new.get(ix.map_ids(ids)) == old.get(ids)
    assert new.get(ix.map_ids(ids), ["url"]) == old.get(ids, ["url"])
    # a column subset, and one file when everything fits
    sub = str(tmp_path / "sub")
    assert len(reorder_arrow_metadata(ix, src, sub, columns=["score", "url", "nope"])) == 1
    subp = ArrowMetadataProvider(sub)
    assert subp.table.schema.names == ["url", "score"] and subp.get(ix.map_ids(ids)) == old.get(ids, ["url", "score"])
    with pytest.raises(ValueError):
        reorder_arrow_metadata(_PermIndex(np.arange(n - 1)), src, str(tmp_path / "bad"))
