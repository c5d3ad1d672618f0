"""Growing a built IVF index (knnx_ivf_append* / knnx_ivf_merge_from) without a GPU: the host plan of csrc/knnx_grow_plan.h driven by a
stand-alone program under the sanitizers, the header's freedom from HIP, the loud failure of the four entry points on a null index, and
append_new_folder_rows refusing a folder whose old files changed before it touches a device."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grow_plan_under_sanitizers(tmp_path):
    """tools/grow_plan_check.cpp (its own main, only knnx_grow_plan.h) built with -fsanitize=address,undefined and run as a child: the
    new layout equals the build's layout of the summed sizes, every old tile is the source of exactly one new tile, the positions of
    appended rows over ragged chunks, an empty index of empty lists, extra counts all zero, one list that takes everything, list ids
    out of range, and the 2^32 padded-row refusal."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "grow_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "clip-retrieval_amd", "csrc"), os.path.join(ROOT, "tools", "grow_plan_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked into the program where the toolchain has them as archives; the toolchain's default otherwise
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert run.stdout.rstrip().endswith("grow plan ok") and "FAILED" not in run.stdout
    for case in ("crafted growth", "extra counts all zero", "empty index of empty lists", "empty index, nothing added",
                 "one list takes everything", "first and last list grow"):
        assert any(ln.startswith("plan " + case) for ln in lines), case
    assert sum(ln.startswith("positions ") for ln in lines) >= 5
    assert any(ln.startswith("positions one list takes everything") for ln in lines)
    assert any(ln.startswith("refusal 2^32 padded rows") for ln in lines)
    assert any(ln.startswith("refusal list id out of range") for ln in lines)


def test_header_has_no_hip():
    text = open(os.path.join(ROOT, "clip-retrieval_amd", "csrc", "knnx_grow_plan.h"), encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes  # system headers only, none of HIP's
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text and "hipError" not in text


def test_entry_points_are_exported_and_refuse_a_null_index(lib):
    """The four symbols are there, and each answers KNNX_E_ARG with a message on a null index, before it touches a device; the
    caller's buffers are left alone."""
    rows = (C.c_uint16 * 256)()
    lists = (C.c_int32 * 1)(7)
    for name, args in (("knnx_ivf_append_assigned", (None, rows, 1, lists)), ("knnx_ivf_append", (None, rows, 1, lists)),
                       ("knnx_ivf_append_device", (None, rows, 1, lists)), ("knnx_ivf_merge_from", (None, None))):
        assert getattr(lib, name)(*args) == -1, name  # KNNX_E_ARG
        msg = lib.knnx_last_error()
        assert b"null" in msg and name.encode() in msg, (name, msg)
    assert list(lists) == [7]


def _write_folder(folder, counts, d=256, seed=0):
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(seed)
    for i, n in enumerate(counts):
        np.save(os.path.join(folder, f"img_emb_{i:04d}.npy"), (0.1 * rng.standard_normal((n, d))).astype(np.float16))


class _NoDevice(SimpleNamespace):
    """Stands where an index would: any attempt to append fails the test."""

    def ivf_append(self, x, lists=None):
        raise AssertionError("append_new_folder_rows reached the index although the folder must be refused")


def test_append_new_folder_rows_refuses_a_changed_folder(tmp_path):
    """The files an index was built from must still be a prefix of the folder, names and row counts: a file that grew, one that was
    renamed, one that vanished, another dimension, an index that does not reach the end of its folder, and an index that was not
    built from a folder are all refused with ValueError before the index is touched."""
    from clip_retrieval_amd.knn import FolderRows, append_new_folder_rows

    folder = str(tmp_path / "emb")
    _write_folder(folder, [40, 25])
    built = FolderRows(folder).manifest()["files"]
    assert built == [["img_emb_0000.npy", 40], ["img_emb_0001.npy", 25]]

    def index(files=built, rng=(0, 65), d=256):
        return _NoDevice(ivf_folder=folder, ivf_folder_files=files, ivf_row_range=rng, d=d, ntotal=rng[1] - rng[0])

    # a third file arrives, but an old file has changed its row count
    _write_folder(folder, [40, 26, 10], seed=1)
    with pytest.raises(ValueError, match="changed"):
        append_new_folder_rows(index())
    # ... its name (the old second file is gone, another one sorts in its place)
    os.remove(os.path.join(folder, "img_emb_0001.npy"))
    np.save(os.path.join(folder, "img_emb_0001b.npy"), np.zeros((25, 256), np.float16))
    with pytest.raises(ValueError, match="changed"):
        append_new_folder_rows(index())
    # ... a file of the build has vanished altogether
    os.remove(os.path.join(folder, "img_emb_0001b.npy"))
    os.remove(os.path.join(folder, "img_emb_0002.npy"))
    with pytest.raises(ValueError, match="changed"):
        append_new_folder_rows(index())
    # the folder is whole again and has gained a file: another dimension, a shard that stops early, no folder on record
    _write_folder(folder, [40, 25, 10])
    with pytest.raises(ValueError, match="changed"):
        append_new_folder_rows(index(d=512))
    with pytest.raises(ValueError, match="reaches the end"):
        append_new_folder_rows(index(rng=(0, 40)))
    with pytest.raises(ValueError, match="built from an embeddings folder"):
        append_new_folder_rows(_NoDevice(d=256, ntotal=65))
    # and the folder given by hand is checked the same way
    other = str(tmp_path / "moved")
    _write_folder(other, [41, 25, 10])
    with pytest.raises(ValueError, match="changed"):
        append_new_folder_rows(index(), folder=other)
