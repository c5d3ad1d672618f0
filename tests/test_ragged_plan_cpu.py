"""The ragged-batch planner of the two text towers (csrc/clipx_ragged_plan.h) without a GPU: tools/ragged_plan_check.cpp drives it
as a stand-alone program under the sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "clip-retrieval_amd", "csrc", "clipx_ragged_plan.h")


def test_planner_under_sanitizers(tmp_path):
    """tools/ragged_plan_check.cpp (its own main, only clipx_ragged_plan.h) built with -fsanitize=address,undefined and run as a
    child: B in 1 .. 40 x T in {1, 2, 77, 128} x four length patterns x every pad 0 .. 255, plus B = 256 at T = 128 and T = 1 with
    255 pad rows, each in a heap block of exactly the capacity the handles allocate -- the lengths sum to the padded row count, the
    pseudo-samples repeat the first longest sample, only the last is shortened, offsets / row map / pooled rows follow, and every
    array equals what the two loops the planner replaced gave."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ragged_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "clip-retrieval_amd", "csrc"), os.path.join(ROOT, "tools", "ragged_plan_check.cpp"), "-o", exe]
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("ragged plan ok") and "FAILED" not in run.stdout
    assert f"{4 * 40 * 4 * 256 + 8} cases, 0 failures" in run.stdout


def test_planner_header_has_no_hip():
    text = open(HEADER, encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes  # system headers only, none of HIP's
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text and "hipError" not in text
