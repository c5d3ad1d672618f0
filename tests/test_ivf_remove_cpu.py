"""Shrinking a built IVF index (knnx_ivf_remove_ids) without a GPU: the integer arithmetic of csrc/knnx_shrink_plan.h driven by a
stand-alone program under the sanitizers, the header's freedom from HIP, the loud failure of the two entry points on a null index, and
the kept / ivf_lists / ivf_row_range bookkeeping of Mi355xIndex.ivf_remove against numpy on a stub that stands for the library."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shrink_plan_under_sanitizers(tmp_path):
    """tools/shrink_plan_check.cpp (its own main, only knnx_shrink_plan.h) built with -fsanitize=address,undefined and run as a child:
    the block-sum scan, masks, positions, dst0 and the new layout, step by step as the device runs them, agree with the sequential
    reference on the crafted layout (with and without an id_base; the crafted set, nothing, everything and one id dead) and on 3000
    random layouts; ids that name no row; the refusals of inconsistent counts."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "shrink_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "clip-retrieval_amd", "csrc"), os.path.join(ROOT, "tools", "shrink_plan_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked into the program where the toolchain has them as archives; the toolchain's default otherwise
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert run.stdout.rstrip().endswith("shrink plan ok") and "FAILED" not in run.stdout
    for case in ("crafted removal, id_base 0", "crafted removal, id_base 1000", "crafted nothing dead", "crafted everything dead",
                 "crafted first id dead", "empty index of empty lists", "ids that name no row", "mask positions",
                 "refusal inconsistent counts", "random layouts: 3000 of 3000"):
        assert any(ln.startswith(case) for ln in lines), case
    crafted = next(ln for ln in lines if ln.startswith("crafted removal, id_base 0"))
    assert "rows 2294 -> 1776" in crafted and "tiles 82 -> 64" in crafted, crafted


def test_header_has_no_hip():
    text = open(os.path.join(ROOT, "clip-retrieval_amd", "csrc", "knnx_shrink_plan.h"), encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all("hip" not in inc for inc in includes), includes
    assert [inc for inc in includes if not inc.startswith("<")] == ['"knnx_grow_plan.h"']  # system headers and the other host plan
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text and "hipError" not in text


def test_entry_points_are_exported_and_refuse_a_null_index(lib):
    """The two symbols are there and typed, and each answers KNNX_E_ARG with a message on a null index, before it touches a device; the
    caller's buffers are left alone."""
    ids = (C.c_int64 * 2)(3, 4)
    got = C.c_int64(-5)
    assert lib.knnx_ivf_remove_ids(None, ids, 2, C.byref(got)) == -1  # KNNX_E_ARG
    msg = lib.knnx_last_error()
    assert b"null" in msg and b"knnx_ivf_remove_ids" in msg, msg
    assert lib.knnx_ivf_remove_stats(None, None, None, None, None, None, None) == -1
    msg = lib.knnx_last_error()
    assert b"null" in msg and b"knnx_ivf_remove_stats" in msg, msg
    assert list(ids) == [3, 4] and got.value == -5
    for name, nargs in (("knnx_ivf_remove_ids", 4), ("knnx_ivf_remove_stats", 7)):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name


class _StubLib:
    """Stands for the library: an index of `ntotal` rows with ids from `base`, removal done with a Python set."""

    def __init__(self, ntotal, base):
        self.ntotal, self.base, self.calls = ntotal, base, []

    def knnx_ntotal(self, _h):
        return self.ntotal

    def knnx_ivf_remove_ids(self, _h, ptr, n, removed):
        ids = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int64)), shape=(n,)).copy() if n else np.zeros(0, np.int64)
        assert (ptr is None) == (n == 0)
        self.calls.append(ids)
        gone = {int(i) for i in ids if self.base <= i < self.base + self.ntotal}
        self.ntotal -= len(gone)
        removed._obj.value = len(gone)  # pylint: disable=protected-access
        return 0


def _stub_index(ntotal, base, lists=None, folder=False):
    from clip_retrieval_amd.knn import Mi355xIndex

    ix = object.__new__(Mi355xIndex)
    ix._lib, ix._h, ix._id_base = _StubLib(ntotal, base), None, base  # pylint: disable=protected-access
    if lists is not None:
        ix.ivf_lists, ix.ivf_row_range = lists, (base, base + ntotal)
    if folder:
        ix.ivf_source, ix.embeddings_folder, ix.ivf_folder, ix.ivf_folder_files = object(), "/emb", "/emb", [["a.npy", ntotal]]
    return ix


@pytest.mark.parametrize("base", [0, 1000])
def test_bookkeeping_against_numpy(base):
    rng = np.random.default_rng(base)
    n = 500
    lists = rng.integers(0, 24, n).astype(np.int32)
    ix = _stub_index(n, base, lists.copy(), folder=True)
    ids = np.concatenate([base + rng.integers(0, n, 120), [-1, base - 1, base + n, base + n + 5]]).reshape(4, 31)
    want = np.setdiff1d(np.arange(base, base + n), ids)
    kept = ix.ivf_remove(ids.astype(np.int32))  # (any integer type, any shape)
    assert kept.dtype == np.int64 and np.array_equal(kept, want) and 0 < len(kept) < n
    assert ix._lib.calls[0].dtype == np.int64 and np.array_equal(ix._lib.calls[0], ids.reshape(-1))  # pylint: disable=protected-access
    assert np.array_equal(ix.ivf_lists, lists[want - base]) and ix.ivf_lists.dtype == np.int32
    assert ix.ivf_row_range == (base, base + len(want))
    assert not any(hasattr(ix, a) for a in ("ivf_source", "embeddings_folder", "ivf_folder", "ivf_folder_files"))
    # the faiss-shaped form counts; ids are positional, so id base + 0 names the first survivor now
    left = lists[want - base]
    assert ix.remove_ids([base, base, base + 2]) == 2
    assert np.array_equal(ix.ivf_lists, np.delete(left, [0, 2])) and ix.ivf_row_range == (base, base + len(want) - 2)
    # nothing to remove: the call still reaches the library, and nothing changes -- the folder binding included
    ix.ivf_folder = "/emb"
    before = ix.ivf_lists.copy()
    assert ix.remove_ids(np.zeros(0, np.int64)) == 0 and ix.remove_ids([-1, base - 1]) == 0
    assert len(ix._lib.calls) == 4 and ix.ivf_folder == "/emb" and np.array_equal(ix.ivf_lists, before)  # pylint: disable=protected-access
    with pytest.raises(TypeError):
        ix.ivf_remove(np.asarray([1.5]))
    assert len(ix._lib.calls) == 4  # pylint: disable=protected-access
    # everything
    kept = ix.ivf_remove(np.arange(base, base + n))
    assert kept.shape == (0,) and ix.ntotal == 0 and ix.ivf_lists.shape == (0,) and ix.ivf_row_range == (base, base)
    # an index that carries neither lists nor a row range
    bare = _stub_index(10, base)
    assert np.array_equal(bare.ivf_remove([base + 3]), base + np.asarray([0, 1, 2, 4, 5, 6, 7, 8, 9]))
    assert not hasattr(bare, "ivf_lists") and not hasattr(bare, "ivf_row_range")
