"""The bookkeeping of the profiler's stamp slots (csrc/clipx_stamp_slots.h: the ids handed out, the runs a read copies back and
refills, the reduction of a slot's entries) and the plans of the GPU tests' shapes, without a GPU: tools/stamp_slots_check.cpp drives it as a stand-alone program
under the sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "clip-retrieval_amd", "csrc", "clipx_stamp_slots.h")


def test_slot_book_under_sanitizers(tmp_path):
    """StampBook over random bursts of hand-outs and reads at six chunk sizes (consecutive ids, a chunk added exactly when the ids
    run out, one run per chunk, reset keeps the chunks); stamp_reduce on filled, half-written and reversed slots; and the shapes of
    tests/test_profile_stamps_gpu.py still plan onto the kernels they are there for: 4-wave, 8-wave, 4-wave + a 128x128 launch,
    128x128 alone, split-K for every GEMM of a B = 1 ViT-B/32 text query, no plan for the refused launch."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "stamp_slots_check")
    base = [cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "clip-retrieval_amd", "csrc"), os.path.join(ROOT, "tools", "stamp_slots_check.cpp"), "-o", exe]
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("stamp slots ok") and "FAILED" not in run.stdout and ", 0 failures" in run.stdout


def test_slot_header_has_no_hip():
    text = open(HEADER, encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes  # system headers only, none of HIP's
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text and "hipError" not in text
