"""OPQ rotation in front of IVF-PQ, the parts that need no GPU: the saved folder's flag / file logic, the float32-numpy side of the
row-rotation band (tests/test_opq_gpu.py holds the kernel to the same band and cap), and the Procrustes step inside a numpy
restatement of the OPQ recipe.  The helpers here are what test_opq_gpu.py imports."""
import json

import numpy as np
import pytest

# ------------------------------------------------------------------------------------------------ row rotation: inputs and band
BAND = 2e-7   # an output is fp16(y64 + e) with |e| <= BAND: ten times the fp32 summation error expected for unit-norm operands
CAP = 0.01    # at most this share of the outputs may differ from fp16(y64)
ROT_CASES = [(d, n) for d in (512, 768, 1024) for n in (1, 33, 5000)]


def unit_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float16)


def random_rotation(d, seed):
    """A random orthonormal f32 [d, d] (Q of a Gaussian matrix)."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))
    return np.ascontiguousarray(q.astype(np.float32))


def rotation_band(y16, A, x16):
    """y16 fp16 [n, d] claimed to be fp16(A x) -> (share of outputs that are not fp16(y64), the largest error e before the rounding
    that explains them: the distance from y64 to the reals that round to the output, number of outputs outside [fp16(y64 - BAND),
    fp16(y64 + BAND)]).  y64 = A @ x in float64.

    The condition: every output is fp16(y64 + e) for some |e| <= BAND.  At the typical magnitude 1 / sqrt(d), where an fp16 step is
    3e-5, that is "fp16(y64), or its fp16 neighbour where y64 lies within BAND of the midpoint between the two".  Stated as an interval
    it also covers the few outputs below 2.4e-4 in magnitude, where an fp16 step (6e-8) is SMALLER than the fp32 summation error: there
    float32 numpy itself lands two steps from fp16(y64) (d = 768, n = 5000: y64 = -9.2078e-05, float32 numpy gives -9.197e-05, e =
    8.7e-08), so "the neighbour" cannot be the rule there; the band on e is the same 2e-7 everywhere."""
    y64 = x16.astype(np.float64) @ A.astype(np.float64).T
    want = y64.astype(np.float16)
    off = (y16.view(np.uint16) != want.view(np.uint16)) & ~((y16 == 0) & (want == 0))  # (+0 / -0: one value)
    lo, hi = (y64 - BAND).astype(np.float16), (y64 + BAND).astype(np.float16)
    outside = int(((y16 < lo) | (y16 > hi) | np.isnan(y16)).sum())
    got = y16[off].astype(np.float64)
    need = np.abs(y64[off] - got) - np.spacing(np.abs(y16[off])).astype(np.float64) / 2
    return float(off.mean()), float(need.max(initial=0.0)), outside


@pytest.mark.parametrize("d,n", ROT_CASES)
def test_float32_numpy_is_inside_the_band_and_the_cap(d, n):
    """Plain float32 numpy on the inputs of the kernel test stays inside the 2e-7 band and the 1 % cap: a kernel that leaves them is
    wrong, not unlucky.  (Measured: at most 0.19 % of the outputs differ from fp16(y64), largest e 8.8e-08.)"""
    x, A = unit_rows(n, d, 100 + d + n), random_rotation(d, d)
    y = (x.astype(np.float32) @ A.T).astype(np.float16)
    share, worst, outside = rotation_band(y, A, x)
    print(f"d={d} n={n}: float32 numpy: {share:.2e} of the outputs differ from fp16(y64), largest error before rounding {worst:.2e}")
    assert outside == 0 and worst <= BAND and share <= CAP


# ------------------------------------------------------------------------------------------------ numpy OPQ recipe
def np_pq_encode(Y, cb):
    """codes u8 [n, M] = argmin_j ||y_m - cb[m][j]||^2 in float64, as |y|^2 - 2 <y, c> + |c|^2 one sub-quantiser at a time (the
    n x M x 256 x ds differences of test_ivfpq_gpu.np_encode never exist at once; the two agree except on near-ties)."""
    M, _, ds = cb.shape
    codes = np.empty((Y.shape[0], M), np.uint8)
    for m in range(M):
        y = Y[:, m * ds:(m + 1) * ds].astype(np.float64)
        c = cb[m].astype(np.float64)
        codes[:, m] = ((y * y).sum(1)[:, None] - 2 * y @ c.T + (c * c).sum(1)[None]).argmin(1)
    return codes


def np_pq_decode(cb, codes):
    return cb[np.arange(cb.shape[0])[None, :], codes].reshape(codes.shape[0], -1)


def np_pq_train(Y, M, niter, seed):
    """The recipe of knn.train_pq_codebooks in numpy: 256 distinct random rows per sub-quantiser, `niter` Lloyd iterations, empty
    clusters re-seeded on random rows between iterations."""
    rng = np.random.default_rng(seed)
    n, d = Y.shape
    ds = d // M
    rows = np.concatenate([np.sort(rng.choice(n, 256, replace=False)) for _ in range(M)]).reshape(M, 256)
    cb = np.stack([Y[rows[m], m * ds:(m + 1) * ds] for m in range(M)]).astype(np.float64)
    for it in range(niter):
        codes = np_pq_encode(Y, cb)
        empty = []
        for m in range(M):
            cnt = np.bincount(codes[:, m], minlength=256)
            s = np.zeros((256, ds))
            np.add.at(s, codes[:, m], Y[:, m * ds:(m + 1) * ds].astype(np.float64))
            nz = cnt > 0
            cb[m, nz] = s[nz] / cnt[nz, None]
            empty += [m * 256 + j for j in np.flatnonzero(~nz)]
        if empty and it < niter - 1:
            for e, r in zip(empty, rng.choice(n, len(empty))):
                cb[e // 256, e % 256] = Y[r, (e // 256) * ds:(e // 256 + 1) * ds]
    return cb.astype(np.float32)


def np_opq(X, M, niter, pq_niter, seed):
    """knn.train_opq in numpy (float32 rotation of the rows, float64 X^T Y): the package's own start matrix and Procrustes step."""
    from clip_retrieval_amd.knn import opq_initial_rotation, opq_procrustes

    X = X.astype(np.float32)
    A = opq_initial_rotation(X.shape[1], seed)
    for it in range(niter):
        Y = (X @ A.T).astype(np.float16).astype(np.float32)
        cb = np_pq_train(Y, M, pq_niter, seed + it)
        dec = np_pq_decode(cb, np_pq_encode(Y, cb))
        A = opq_procrustes(X.astype(np.float64).T @ dec.astype(np.float64))
    return A


def quantisation_error(Y, cb):
    """mean squared distance between a row and its decode"""
    Y = Y.astype(np.float32)
    return float(((Y - np_pq_decode(cb, np_pq_encode(Y, cb))) ** 2).sum(1).mean())


def heavy_rows(n, d, seed, heavy=16, scale=6.0):
    """The dominant-column corpus of the int8 stage (oracle synth_rows(..., dominant=True): three columns with 6 x the spread and a
    common offset) with the next heavy - 3 columns scaled by `scale` too, re-normalised, fp16: the leading `heavy` columns -- one PQ
    slice at d / M = 16 -- carry most of the variance.  (Kind 2 as it is gives a plain PQ nothing to lose: three columns whose large
    part is a CONSTANT cost one sub-quantiser little, and a numpy OPQ does not beat numpy PQ on it -- error 0.440 against 0.419 at
    n = 6000, d = 512, M = 32.  With 16 heavy columns: error 0.339 against 0.483, recall@10 0.67 against 0.22.)"""
    from oracle.knn_oracle import synth_rows

    x = synth_rows(np.arange(n), d, seed, dominant=True).astype(np.float32)
    x[:, 3:heavy] *= scale
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float16)


def test_procrustes_step_on_a_planted_rotation():
    """Rows = a known rotation of data whose variance sits in 8 of 64 columns: the numpy recipe with the package's Procrustes step
    returns an orthonormal matrix under which PQ loses less than under the identity."""
    from clip_retrieval_amd.knn import opq_procrustes

    n, d, M = 3000, 64, 8
    rng = np.random.default_rng(0)
    z = rng.standard_normal((n, d)).astype(np.float32)
    z[:, :8] *= 6.0
    R0 = random_rotation(d, 1)
    x = ((z / np.linalg.norm(z, axis=1, keepdims=True)) @ R0.T).astype(np.float16)
    # the Procrustes step alone recovers a planted rotation exactly: Y = X R0^T  ->  A = R0
    xs = x.astype(np.float64)
    B = random_rotation(d, 2)
    assert np.abs(opq_procrustes(xs.T @ (xs @ B.astype(np.float64).T)) - B).max() < 1e-5
    A = np_opq(x, M, niter=6, pq_niter=4, seed=0)
    assert np.abs(A @ A.T - np.eye(d)).max() < 1e-4
    xf = x.astype(np.float32)
    e_id = quantisation_error(xf, np_pq_train(xf, M, 4, 9))
    y = xf @ A.T
    e_opq = quantisation_error(y, np_pq_train(y, M, 4, 9))
    print(f"quantisation error: identity {e_id:.5f}, OPQ {e_opq:.5f}")
    assert e_opq < e_id


# ------------------------------------------------------------------------------------------------ saved folder
def test_manifest_flag_and_rotation_file_go_together(tmp_path):
    from clip_retrieval_amd import knn

    d = 8
    rot = random_rotation(d, 3)
    old = {"format": knn.IVFPQ_FORMAT, "d": d, "nlist": 2, "M": 16, "nprobe": 1, "row_range": [0, 4]}
    # a folder written before the rotation existed: no key, no file
    assert knn.read_ivfpq_rotation(str(tmp_path), old) is None
    assert knn.read_ivfpq_rotation(str(tmp_path), dict(old, opq=False)) is None
    # the flag without the file
    with pytest.raises(ValueError, match="ivf_pq_rotation.npy is missing"):
        knn.read_ivfpq_rotation(str(tmp_path), dict(old, opq=True))
    np.save(tmp_path / knn.IVFPQ_ROTATION, rot)
    # flag and file
    assert np.array_equal(knn.read_ivfpq_rotation(str(tmp_path), dict(old, opq=True)), rot)
    # the file without the flag: somebody's rotation would be silently dropped
    with pytest.raises(ValueError, match="does not say"):
        knn.read_ivfpq_rotation(str(tmp_path), old)
    # a matrix of another shape or type
    np.save(tmp_path / knn.IVFPQ_ROTATION, rot[:4])
    with pytest.raises(ValueError, match="must be float32"):
        knn.read_ivfpq_rotation(str(tmp_path), dict(old, opq=True))
    np.save(tmp_path / knn.IVFPQ_ROTATION, rot.astype(np.float64))
    with pytest.raises(ValueError, match="must be float32"):
        knn.read_ivfpq_rotation(str(tmp_path), dict(old, opq=True))
    json.dumps(old)  # (the manifest stays plain JSON)


def test_rotation_padding_is_the_identity_on_the_pad_columns():
    from clip_retrieval_amd.knn import _pad_rotation

    A = random_rotation(5, 4)
    P = _pad_rotation(A, 8)
    assert P.shape == (8, 8) and np.array_equal(P[:5, :5], A) and np.array_equal(P[5:, 5:], np.eye(3, dtype=np.float32))
    assert not P[:5, 5:].any() and not P[5:, :5].any()
    assert _pad_rotation(A, 5) is not None and np.array_equal(_pad_rotation(A, 5), A)
