"""The split Huffman decode inside a restart interval without a GPU (`huffman_split`): csrc/jpegx_split.h run on the CPU
under the sanitizers against the serial interval decoder, the host entry of the C ABI against the host entropy stage, and the switch
through reader and worker."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_inputs as J
import jpeg_split_inputs as SI
from test_jpeg_huffman_cpu import mutants

ROOT = J.ROOT
CSRC = os.path.join(ROOT, "clip-retrieval_amd", "csrc")
INTERVAL = np.dtype([("first_mcu", "<i4"), ("nmcu", "<i4"), ("begin", "<u4"), ("end", "<u4")])


def all_files():
    return J.cases() + SI.cases()


def longest_interval(packed):
    """Entropy-coded bytes of the longest restart interval of a jpeg.scan_packed() array."""
    from clip_retrieval_amd import jpeg

    rec = packed[64:]
    h = rec[:64].view(jpeg.SCAN_HEADER)[0]
    at = 64 + jpeg.TABLE_BYTES + int(h["ntables"]) * jpeg.HUFF_BYTES
    ivl = rec[at:at + int(h["nintervals"]) * 16].view(INTERVAL)
    return int((ivl["end"].astype(np.int64) - ivl["begin"]).max())


def test_inputs_cover_the_cases_of_the_cut():
    """The new set: no restart markers, at most 60 KB, every content with every sampling and quality in some file; together with the
    146 files: an interval of exactly 2 sub-sequences, hundreds of blocks per sub-sequence, blocks longer than a sub-sequence."""
    from clip_retrieval_amd import jpeg

    files = SI.cases()
    assert 36 <= len(files) <= 50 and len({n for n, _ in files}) == len(files)
    assert all(len(d) <= SI.MAX_BYTES and jpeg.scan_packed(d)[64:128].view(jpeg.SCAN_HEADER)[0]["nintervals"] == 1 for _, d in files)
    for kind in SI.CONTENTS:
        assert len({n.split("-")[1] for n, _ in files if f"-{kind}-" in n}) == 4, kind  # every sampling
    sizes = {n: longest_interval(jpeg.scan_packed(d)) for n, d in all_files()}
    assert sizes[SI.two_subsequences()[0]] == 64  # exactly two sub-sequences at 32
    big = [d for n, d in files if n.startswith("256x256") and "-flat-" in n]
    assert big and min(len(d) for d in big) < 1536  # 1 024+ blocks in under 1.5 KB: hundreds of blocks per 128-byte sub-sequence
    assert any("-noise-q100-" in n or "-noise-q95-" in n for n, _ in files)  # blocks of far more than 32 bytes


def test_split_decoder_under_sanitizers(tmp_path):
    """tools/jpeg_split_check.cpp (its own main, only the headers) built with -fsanitize=address,undefined and run as a child over the
    146 accepted files, the no-restart-marker set and the 2 000 seeded mutants.  Per prepared file, split_bytes in {32, 128, 1024} and
    max_rounds in {1, 4096}: every interval's code equals the serial decoder's, records are byte-equal when clean, rounds is 0 / -1 /
    2 .. sub-sequences + 1 as the interval's size and the cap say."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    files = tmp_path / "files"
    files.mkdir()
    for i, (_, data) in enumerate(J.cases()):
        (files / f"a{i:04d}.bin").write_bytes(data)
    for i, (_, data) in enumerate(SI.cases()):
        (files / f"n{i:04d}.bin").write_bytes(data)
    for i, data in enumerate(mutants()):
        (files / f"m{i:04d}.bin").write_bytes(data)
    exe = str(tmp_path / "jpeg_split_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            os.path.join(ROOT, "tools", "jpeg_split_check.cpp"), "-o", exe]
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe, str(files)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("jpeg split ok") and "FAILED" not in run.stdout
    counts = {ln.split()[1]: [int(x) for x in ln.split()[2:]] for ln in run.stdout.splitlines() if ln.startswith("prefix ")}
    print(counts)  # files, prepared, split intervals at 32 bytes, most rounds at 32 bytes
    assert counts["a"][:2] == [146, 146] and counts["n"][:2] == [len(SI.cases())] * 2 and counts["m"][0] == 2000
    assert counts["a"][2] >= 500 and counts["n"][2] >= 36 and counts["m"][1] >= 1400 and counts["m"][2] >= 900  # the cut is taken
    assert counts["n"][3] >= 64  # content that never synchronises: as many rounds as sub-sequences


def test_header_has_no_hip_and_is_in_the_makefile():
    text = open(os.path.join(CSRC, "jpegx_split.h"), encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ['"jpegx_scan.h"'], includes
    for word in ("__global__", "__device__", "__shared__", "hipStream", "hipError", "hipMalloc", "hipMemcpy", "hipLaunch", "<<<", "hip_runtime", "asm"):
        assert word not in text, word
    mk = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    assert "jpegx_split.h" in mk and "jpeg_split_kernels.hip" in mk and "jpeg_huff_dev.h" in mk
    kernel = open(os.path.join(CSRC, "jpeg_split_kernels.hip"), encoding="utf-8").read()
    assert "huff_split_kernel" in kernel and "asm" not in kernel
    tool = open(os.path.join(ROOT, "tools", "jpeg_split_check.cpp"), encoding="utf-8").read()
    assert "int main(" in tool and "hip_runtime" not in tool and "clipx.h" not in tool


@pytest.mark.parametrize("split", (32, 128))
def test_host_entry_equals_the_host_stage(lib, split):
    """clipx_jpeg_entropy_split_host over every file: the record is jpeg.entropy()'s byte for byte; with max_rounds 4096 no image
    falls back and an image reports rounds >= 2 exactly when one of its intervals has 2 x split bytes; with max_rounds 1 exactly
    those report -1, and the records are still equal."""
    from clip_retrieval_amd import jpeg

    nsplit = 0
    for name, data in all_files():
        packed = jpeg.scan_packed(data, lib=lib)
        want = jpeg.entropy(data, lib=lib)
        assert packed is not None and want is not None, name
        is_split = longest_interval(packed) >= 2 * split
        nsplit += is_split
        for cap in (4096, 1):
            status, rec, rounds = jpeg.entropy_split_host(packed[64:], packed[:64].view(jpeg.JPEG_DESC), split, cap, lib=lib)
            assert status == 0, (name, cap, status)
            assert rec.size == want[1].size and np.array_equal(rec, want[1]), f"{name}: the record differs from the host stage's (cap {cap})"
            if cap == 1:
                assert rounds == (-1 if is_split else 0), (name, rounds)
            else:
                assert (rounds >= 2) if is_split else (rounds == 0), (name, rounds)
    assert nsplit >= (100 if split == 32 else 30), nsplit


def test_host_entry_switch_off_default_and_bad_values(lib):
    from clip_retrieval_amd import jpeg

    for name, data in all_files()[::7]:
        packed = jpeg.scan_packed(data, lib=lib)
        desc = packed[:64].view(jpeg.JPEG_DESC)
        status, rec, rounds = jpeg.entropy_split_host(packed[64:], desc, 0, lib=lib)
        assert (status, rounds) == (0, 0) and np.array_equal(rec, jpeg.entropy(data, lib=lib)[1]), name
        status, rec, rounds = jpeg.entropy_split_host(packed[64:], desc, 64, lib=lib)  # the default cap
        assert status == 0 and np.array_equal(rec, jpeg.entropy(data, lib=lib)[1]), name
    packed = jpeg.scan_packed(all_files()[0][1], lib=lib)
    rec = np.ascontiguousarray(packed[64:]).copy()
    desc = packed[:64].copy()
    out = np.zeros(jpeg.record_bytes(desc.view(jpeg.JPEG_DESC)[0]), dtype=np.uint8)
    status, rounds = C.c_int32(77), C.c_int32(77)
    for bad in (3, 16, 2048, -32, 48):
        with pytest.raises(ValueError):
            jpeg.entropy_split_host(packed[64:], desc.view(jpeg.JPEG_DESC), bad, lib=lib)
        arg = np.zeros(1, dtype=jpeg.JPEG_SPLIT)
        arg["split_bytes"] = bad
        rc = lib.clipx_jpeg_entropy_split_host(rec.ctypes.data, rec.size, desc.ctypes.data, arg.ctypes.data, out.ctypes.data, out.size,
                                               C.byref(status), C.byref(rounds))
        assert rc < 0 and (status.value, rounds.value) == (77, 77) and not out.any(), bad
    arg = np.zeros(1, dtype=jpeg.JPEG_SPLIT)
    arg["split_bytes"], arg["max_rounds"] = 32, -1
    assert lib.clipx_jpeg_entropy_split_host(rec.ctypes.data, rec.size, desc.ctypes.data, arg.ctypes.data, out.ctypes.data, out.size,
                                             C.byref(status), C.byref(rounds)) < 0


def test_malformed_files_get_the_host_stages_verdict(lib):
    """The first 600 mutants through the host entry at split 32: status 0 exactly where jpeg.entropy() takes the file, and then the
    same record."""
    from clip_retrieval_amd import jpeg

    refused = 0
    for i, m in enumerate(mutants(600)):
        packed = jpeg.scan_packed(m, lib=lib)
        if packed is None:
            continue
        want = jpeg.entropy(m, lib=lib)
        status, rec, _ = jpeg.entropy_split_host(packed[64:], packed[:64].view(jpeg.JPEG_DESC), 32, 4096, lib=lib)
        assert (status == 0) == (want is not None) and 0 <= status <= 7, (i, status)
        if want is not None:
            assert np.array_equal(rec, want[1]), i
        refused += status != 0
    assert refused >= 80


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def _raw(key, data):
    return {"key": key, "image": data, "text": None, "metadata": None}


def test_switch_travels_in_the_batch_only_when_it_is_on(lib):
    from clip_retrieval_amd import reader as R
    from clip_retrieval_amd.worker import worker

    with pytest.raises(ValueError):
        R.DecodeRgbU8(224, huffman_split=128)
    with pytest.raises(ValueError):
        R.DecodeRgbU8(224, gpu_jpeg=True, huffman_split=128)
    with pytest.raises(ValueError):
        R.DecodeRgbU8(224, gpu_huffman=True, huffman_split=100)
    off, on = R.DecodeRgbU8(224, gpu_huffman=True), R.DecodeRgbU8(224, gpu_huffman=True, huffman_split=128)
    assert off.huffman_split == 0 and on.huffman_split == 128 and R.DecodeRgbU8.huffman_split == 0 and R.DecodeRgbU8(224).huffman_split == 0
    files = [d for _, d in SI.cases()[-3:]]
    s_off = [R._decode_sample(_raw(str(i), d), off, None, True, False, False) for i, d in enumerate(files)]
    s_on = [R._decode_sample(_raw(str(i), d), on, None, True, False, False) for i, d in enumerate(files)]
    for a, b in zip(s_off, s_on):  # the samples are the same
        assert sorted(a) == sorted(b) == ["image_filename", "image_jpeg_scan"] and np.array_equal(a["image_jpeg_scan"], b["image_jpeg_scan"])
    b_off = R._collate(s_off, True, False, False, False)
    b_zero = R._collate(s_on, True, False, False, False, 0)
    b_on = R._collate(s_on, True, False, False, False, on.huffman_split)
    keys = ["coef_bytes", "descs", "names", "offs", "scans", "slots"]
    assert sorted(b_off["image_jpeg_scan"]) == sorted(b_zero["image_jpeg_scan"]) == keys
    assert sorted(b_on["image_jpeg_scan"]) == sorted(keys + ["split_bytes"]) and b_on["image_jpeg_scan"]["split_bytes"] == 128
    for k in keys:
        x, y = b_off["image_jpeg_scan"][k], b_on["image_jpeg_scan"][k]
        assert (np.array_equal(np.asarray(x), np.asarray(y)) if k != "descs" else x.tobytes() == y.tobytes()), k
    assert np.array_equal(b_off["image_raw"]["offsets"], b_on["image_raw"]["offsets"]) and np.array_equal(b_off["image_raw"]["hw"], b_on["image_raw"]["hw"])
    # a batch without scans never carries the key
    plain = [R._decode_sample(_raw("p", files[0]), R.DecodeRgbU8(224), None, True, False, False)]
    assert sorted(R._collate(plain, True, False, False, False, 128)) == ["image_filename", "image_raw"]
    # worker(): the argument exists, is off, and is refused without gpu_huffman before anything is loaded
    assert inspect.signature(worker).parameters["gpu_huffman_split"].default == 0
    with pytest.raises(ValueError):
        worker(tasks=[0], input_dataset=[], output_folder="unused", output_partition_count=1, gpu_huffman_split=128)
