"""The GEMM planner of the encode half (csrc/clipx_gemm_plan.h) without a GPU: tools/gemm_plan_check.cpp drives it as a stand-alone
program under the sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "clip-retrieval_amd", "csrc", "clipx_gemm_plan.h")

# M: 1 .. 600, every multiple of 256 up to 66 048 with its two neighbours (six of those lie inside 1 .. 600; 65 792 is one of the
# multiples), and 10 547
N_M = 600 + 3 * 258 - 6 + 1
# x N (10) x K (8) x n_cu (5) x epilogue (8) x f16 (2) x variant (7) x row0 (2) x statistics (2) x split-K scratch (3)
N_CASES = N_M * 10 * 8 * 5 * 8 * 2 * 7 * 2 * 2 * 3


def test_plan_under_sanitizers(tmp_path):
    """tools/gemm_plan_check.cpp (its own main, only clipx_gemm_plan.h) built with -fsanitize=address,undefined and run as a child:
    the full cross product of M x N x K x epilogue x operand type x variant x n_cu x row0 x statistics x split-K scratch.  Every
    case gives the list of launches the code the plan replaced gave (restated in the tool as it was), the four gemm256_* functions,
    the split-K factor and the two predicates of the 4-wave kernel equal their old forms, the row ranges partition [0, M), tail_nb
    is 1 .. 4 and divides N / 32, the strips fit the grid, and statistics rows plus fused rows are M."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gemm_plan_check")
    base = [cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I",
            os.path.join(ROOT, "clip-retrieval_amd", "csrc"), os.path.join(ROOT, "tools", "gemm_plan_check.cpp"), "-o", exe]
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("gemm plan ok") and "FAILED" not in run.stdout
    assert f"gemm plan: {N_CASES} cases" in run.stdout and ", 0 failures" in run.stdout
    assert "more tail strips than workgroups that own a bulk tile" in run.stdout  # printed, never a failure


def test_plan_header_has_no_hip():
    text = open(HEADER, encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes  # system headers only, none of HIP's
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text and "hipError" not in text
