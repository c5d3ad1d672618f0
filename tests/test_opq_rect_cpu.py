"""OPQ with d_out > d_in (faiss OPQMatrix(d_in, M, d_out), "OPQ256_768" on 512-d rows), the parts that need no GPU: the width rule and
the column-Gram check (csrc/knnx_rot_shape.h) under the sanitizers, the saved folder's "d_out" logic, the index-key parser, the numpy
statement of rectangular training, and the float32-numpy side of the row-rotation band for rectangular matrices
(tests/test_opq_rect_gpu.py holds the kernel to the same band and cap).  RECT_PAIRS and rect_rotation are what that file imports."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_opq_cpu import BAND, CAP, np_opq, np_pq_train, quantisation_error, random_rotation, rotation_band, unit_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECT_PAIRS = [(256, 512), (256, 768), (256, 1024), (512, 768), (512, 1024), (768, 1024)]  # every supported (d_in, d_out)


def rect_rotation(d_in, d_out, seed=None):
    """(A_sq f32 [d_out, d_out] orthonormal, A = its first d_in columns, f32 [d_out, d_in] with orthonormal columns)"""
    A_sq = random_rotation(d_out, d_out if seed is None else seed)
    return A_sq, np.ascontiguousarray(A_sq[:, :d_in])


# ------------------------------------------------------------------------------------------------ the header under the sanitizers
def test_rot_shape_under_sanitizers(tmp_path):
    """tools/rot_shape_check.cpp (its own main, only knnx_rot_shape.h) built with -fsanitize=address,undefined and run as a child:
    every supported and every refused pair of widths, an orthonormal rectangular matrix of every pair, one with a scaled column, one
    with a NaN, and a square matrix by rows and by columns."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "rot_shape_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "clip-retrieval_amd", "csrc"), os.path.join(ROOT, "tools", "rot_shape_check.cpp"), "-o", exe]
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("rot shape ok") and "FAILED" not in run.stdout
    lines = run.stdout.splitlines()
    assert sum(ln.startswith("shape ") and ln.endswith("supported") for ln in lines) == 10
    assert sum(ln.startswith("shape ") and ln.endswith("refused") for ln in lines) >= 20
    assert sum(ln.startswith("gram rect") for ln in lines) >= 8 and sum(ln.startswith("gram square") for ln in lines) == 2


def test_rot_shape_header_has_no_hip():
    text = open(os.path.join(ROOT, "clip-retrieval_amd", "csrc", "knnx_rot_shape.h"), encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text and "hipError" not in text


# ------------------------------------------------------------------------------------------------ saved folder
def test_manifest_d_out_and_rotation_shape_go_together(tmp_path):
    from clip_retrieval_amd import knn

    d, dq = 256, 512
    _, rot = rect_rotation(d, dq, 3)
    old = {"format": knn.IVFPQ_FORMAT, "d": d, "nlist": 2, "M": 16, "nprobe": 1, "row_range": [0, 4], "opq": True}
    # what save_index writes: the key only when the widths differ
    assert knn.ivfpq_out_dim_entry(d, d) == {} and knn.ivfpq_out_dim_entry(d, dq) == {"d_out": dq}
    assert knn.read_ivfpq_out_dim(str(tmp_path), old) == d and knn.read_ivfpq_out_dim(str(tmp_path), dict(old, d_out=dq)) == dq
    # round trip: key and shape
    np.save(tmp_path / knn.IVFPQ_ROTATION, rot)
    got = knn.read_ivfpq_rotation(str(tmp_path), dict(old, d_out=dq))
    assert got.shape == (dq, d) and np.array_equal(got, rot)
    json.dumps(dict(old, **knn.ivfpq_out_dim_entry(d, dq)))  # (the manifest stays plain JSON)
    # the shape without the key: today's message, today's shape
    with pytest.raises(ValueError, match=rf"must be float32 \[{d}, {d}\]"):
        knn.read_ivfpq_rotation(str(tmp_path), old)
    # the key without the right shape: a square file, and a rectangular one of another d_out
    np.save(tmp_path / knn.IVFPQ_ROTATION, random_rotation(d, 4))
    with pytest.raises(ValueError, match=rf"must be float32 \[{dq}, {d}\]"):
        knn.read_ivfpq_rotation(str(tmp_path), dict(old, d_out=dq))
    np.save(tmp_path / knn.IVFPQ_ROTATION, rect_rotation(d, 768, 5)[1])
    with pytest.raises(ValueError, match=rf"must be float32 \[{dq}, {d}\]"):
        knn.read_ivfpq_rotation(str(tmp_path), dict(old, d_out=dq))
    # the transposed matrix is not the matrix
    np.save(tmp_path / knn.IVFPQ_ROTATION, np.ascontiguousarray(rot.T))
    with pytest.raises(ValueError, match="must be float32"):
        knn.read_ivfpq_rotation(str(tmp_path), dict(old, d_out=dq))
    # keys that obey no width rule, and the key without "opq"
    np.save(tmp_path / knn.IVFPQ_ROTATION, rot)
    for bad in (700, 128, d, 1280, "512", True, 512.0):
        with pytest.raises(ValueError, match="d_out"):
            knn.read_ivfpq_rotation(str(tmp_path), dict(old, d_out=bad))
    with pytest.raises(ValueError, match="d_out"):
        knn.read_ivfpq_out_dim(str(tmp_path), dict(old, d=100, d_out=256))
    os.remove(tmp_path / knn.IVFPQ_ROTATION)
    plain = {k: v for k, v in old.items() if k != "opq"}
    with pytest.raises(ValueError, match="does not say"):
        knn.read_ivfpq_rotation(str(tmp_path), dict(plain, d_out=dq))
    assert knn.read_ivfpq_rotation(str(tmp_path), plain) is None


# ------------------------------------------------------------------------------------------------ index keys
def test_index_key_of_the_notebook():
    from clip_retrieval_amd.knn import ivfpq_params_from_index_key as parse

    assert parse("OPQ256_768,IVF16384_HNSW32,PQ256x8", 512) == {"nlist": 16384, "M": 256, "opq": True, "opq_dim": 768, "refine": False}
    assert parse("OPQ256_768,IVF16384,PQ256x8,RFlat", 512)["refine"] is True
    assert parse("OPQ64_768,IVF4096,PQ64x8", 768) == {"nlist": 4096, "M": 64, "opq": True, "opq_dim": None, "refine": False}
    assert parse("OPQ32,IVF100,PQ32", 512) == {"nlist": 100, "M": 32, "opq": True, "opq_dim": None, "refine": False}
    assert parse("IVF65536_HNSW32,PQ64x8", 1024) == {"nlist": 65536, "M": 64, "opq": False, "opq_dim": None, "refine": False}


@pytest.mark.parametrize("key,d,part", [
    ("OPQ256_700,IVF16384_HNSW32,PQ256x8", 512, "OPQ256_700"),    # a width that is no multiple of 256
    ("OPQ256_512,IVF16384_HNSW32,PQ256x8", 768, "OPQ256_512"),    # d_out < d
    ("OPQ256_1280,IVF16384,PQ256x8", 512, "OPQ256_1280"),         # d_out > 1024
    ("OPQ256_768,IVF16384,PQ256x8", 500, "OPQ256_768"),           # d % 256 != 0 with d_out != d
    ("OPQ64_768,IVF16384,PQ256x8", 512, "OPQ64_768"),             # the OPQ's M is not the PQ's
    ("OPQ256_768,IVF16384,PQ256x4", 512, "PQ256x4"),              # 4-bit codes
    ("OPQ256_768,IVF16384,PQ48x8", 512, "PQ48x8"),                # an M no kernel serves
    ("IVF16384,PQ256x8", 256, "PQ256x8"),                         # M = 256 needs a quantiser width of 512 at least
    ("OPQ256_768,HNSW32,PQ256x8", 512, "HNSW32"),                 # a graph index
    ("OPQ256_768,IVF16384,Flat", 512, "Flat"),                    # no PQ
    ("OPQ256_768,IVF16384,PQ256x8,Refine(Flat)", 512, "Refine"),  # a part nobody serves
    ("PCA256,IVF16384,PQ64x8", 512, "PCA256"),
    ("", 512, "IVF"),
])
def test_index_key_refusals(key, d, part):
    from clip_retrieval_amd.knn import ivfpq_params_from_index_key as parse

    with pytest.raises(ValueError, match=part.replace("(", r"\(")):
        parse(key, d)


# ------------------------------------------------------------------------------------------------ rectangular training in numpy
def np_opq_rect(X, M, d_out, niter, pq_niter, seed):
    """knn.train_opq(d_out=) in numpy: the sample zero-padded to d_out, the square recipe at d_out, the first d_in columns kept."""
    Xp = np.zeros((X.shape[0], d_out), np.float32)
    Xp[:, : X.shape[1]] = X
    return np.ascontiguousarray(np_opq(Xp, M, niter, pq_niter, seed)[:, : X.shape[1]])


def test_rectangular_training_in_numpy():
    """n = 3 000, d_in = 64, d_out = 96, M = 8, rows whose variance sits in 8 columns behind a planted rotation: the kept columns are
    orthonormal to 1e-5 (the matrix's ROWS are not), two runs give the same bits, and PQ in the rotated d_out space loses less than PQ
    of the rows zero-embedded into d_out.  (Measured: zero-embedding 0.229, PQ in d_in 0.178, rectangular OPQ 0.136.)"""
    n, d, dq, M = 3000, 64, 96, 8
    rng = np.random.default_rng(0)
    z = rng.standard_normal((n, d)).astype(np.float32)
    z[:, :8] *= 6.0
    x = ((z / np.linalg.norm(z, axis=1, keepdims=True)) @ random_rotation(d, 1).T).astype(np.float16)
    A = np_opq_rect(x, M, dq, niter=6, pq_niter=4, seed=0)
    assert A.shape == (dq, d) and A.dtype == np.float32
    A64 = A.astype(np.float64)
    cols, rows = np.abs(A64.T @ A64 - np.eye(d)).max(), np.abs(A64 @ A64.T - np.eye(dq)).max()
    print(f"max |A^T A - I| = {cols:.2e}, max |A A^T - I| = {rows:.2f}")
    assert cols <= 1e-5 and rows > 0.5
    assert np.array_equal(A.view(np.uint32), np_opq_rect(x, M, dq, niter=6, pq_niter=4, seed=0).view(np.uint32))
    xf = x.astype(np.float32)
    xp = np.zeros((n, dq), np.float32)
    xp[:, :d] = xf
    e_embed = quantisation_error(xp, np_pq_train(xp, M, 4, 9))
    e_in = quantisation_error(xf, np_pq_train(xf, M, 4, 9))
    y = xf @ A.T
    e_rect = quantisation_error(y, np_pq_train(y, M, 4, 9))
    print(f"quantisation error: zero-embedding {e_embed:.5f}, PQ in d_in {e_in:.5f}, rectangular OPQ {e_rect:.5f}")
    assert e_rect < e_embed


# ------------------------------------------------------------------------------------------------ row rotation: the band
@pytest.mark.parametrize("n", [1, 33, 5000])
@pytest.mark.parametrize("d_in,d_out", RECT_PAIRS)
def test_float32_numpy_is_inside_the_band_and_the_cap_rect(d_in, d_out, n):
    """Plain float32 numpy on the inputs of the rectangular kernel test stays inside test_opq_cpu's 2e-7 band and 1 % cap.
    (Measured over the six pairs x three n: nothing outside the band, largest e 7.6e-08, largest share 0.39 %.)"""
    x = unit_rows(n, d_in, 100 + d_in + d_out + n)
    _, A = rect_rotation(d_in, d_out)
    y = (x.astype(np.float32) @ A.T).astype(np.float16)
    assert y.shape == (n, d_out)
    share, worst, outside = rotation_band(y, A, x)
    print(f"d_in={d_in} d_out={d_out} n={n}: float32 numpy: {share:.2e} of the outputs differ from fp16(y64), largest error {worst:.2e}")
    assert outside == 0 and worst <= BAND and share <= CAP
