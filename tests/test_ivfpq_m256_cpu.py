"""IVF-PQ with M = 256 without a GPU: the planner of the partial-sum buffer (csrc/knnx_pq_plan.h) driven by a stand-alone program under
the sanitizers, the header's freedom from HIP, and the fp32 argument the two-half scan rests on -- a chain of additions cut at m = 128,
stored as float32 and continued is the uncut chain, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_under_sanitizers(tmp_path):
    """tools/pq_plan_check.cpp (its own main, only knnx_pq_plan.h) built with -fsanitize=address,undefined and run as a child: S for
    sizes with ties, zeros, np = 1, np = nlist and np above the non-empty lists; the sub-group cuts at budgets of one byte, exactly one
    slab, nq x S x 4 and one byte less; the ranges tile [0, nq); sizes beyond 2^32 bytes do not wrap."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pq_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "clip-retrieval_amd", "csrc"), os.path.join(ROOT, "tools", "pq_plan_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked into the program where the toolchain has them as archives (nothing then depends on the order in
    # which shared libraries are loaded); the toolchain's default otherwise
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("plan ok") and "FAILED" not in run.stdout
    assert sum(ln.startswith("slab ") for ln in run.stdout.splitlines()) >= 15
    assert sum(ln.startswith("plan ") for ln in run.stdout.splitlines()) >= 15


def test_planner_header_has_no_hip():
    text = open(os.path.join(ROOT, "clip-retrieval_amd", "csrc", "knnx_pq_plan.h"), encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes  # system headers only, none of HIP's
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text and "hipError" not in text


def _chain(lut, codes, m0, m1, start):
    """acc = start; acc += lut[m][codes[:, m]] for m = m0 .. m1 - 1, every addition rounded to float32 (one chain per row)."""
    acc = start.astype(np.float32).copy()
    for m in range(m0, m1):
        acc = (acc + lut[m][codes[:, m]]).astype(np.float32)
    return acc


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_chain_cut_at_128_is_the_uncut_chain(seed):
    """score = cs + acc with acc ONE fp32 sum over m = 0 .. 255 from 0.f (include/knnx.h).  The lower half stores its partial sum as
    float32 and the upper half starts from it: the same additions in the same order, so the same bits -- and not the bits of two
    half-sums added at the end, which is what the scheme must not be confused with."""
    rng = np.random.default_rng(seed)
    n = 4000
    lut = (rng.standard_normal((256, 256)) * 10.0 ** rng.uniform(-3, 1, (256, 1))).astype(np.float32)
    codes = rng.integers(0, 256, (n, 256), dtype=np.uint8)
    zero = np.zeros(n, np.float32)
    whole = _chain(lut, codes, 0, 256, zero)
    lower = _chain(lut, codes, 0, 128, zero)
    stored = np.frombuffer(lower.tobytes(), dtype=np.float32)  # the 4-byte store and load
    assert stored.dtype == np.float32 and np.array_equal(stored.view(np.uint32), lower.view(np.uint32))
    upper = _chain(lut, codes, 128, 256, stored)
    assert np.array_equal(upper.view(np.uint32), whole.view(np.uint32))
    two_sums = (lower + _chain(lut, codes, 128, 256, zero)).astype(np.float32)
    assert (two_sums.view(np.uint32) != whole.view(np.uint32)).any()
