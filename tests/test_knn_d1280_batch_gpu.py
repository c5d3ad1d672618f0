"""Flat kNN at width 1280 in one-pass batches: the register-stationary fp16 scan over a ring of 16-row half tiles
(knn_rq16_scan_kernel<80, 4, 3>, 128 queries per pass) and the int8 first stage at KS = 40, against oracle.knn_oracle.FlatIPOracle
(float64 on the same fp16 rows) under test_knn_gpu._check's tolerance.  Every test runs in both forms.  A failed proof sends a query to
the exact 32-query scan, which would hide a broken kernel, so the counters are part of every test: ix.stats()[0] must rise by exactly
the queries the dispatch gives to a proof-based pass (_served), ix.i8_served() exactly in the int8 form, and ix.stats()[1] must not
move where the data allow it.  Before these kernels existed the counters stayed at 0 at this width."""
import numpy as np
import pytest

from test_knn_gpu import NEG, _check, _data, _queries

pytestmark = pytest.mark.gpu
D = 1280


@pytest.fixture(params=["fp16", "int8"])
def form(monkeypatch, request):
    monkeypatch.setenv("KNNX_RQ_MIN_ROWS", "0")  # read by knnx_create
    monkeypatch.setenv("KNNX_I8", "0" if request.param == "fp16" else "1")
    return request.param


def _served(nq, k, form):
    """queries of one search call that a proof-based pass serves (choose_step, as at d = 1024): none above k = 48 (KNN_WIDE_MAX_K: the
    proofs need a margin below J = 64); the int8 stage takes steps of up to 256 except one of 25 .. 32 queries (measured at this width:
    no faster than one exact scan); the fp16 pass takes steps of up to 128 while more than 64 remain; what is left goes to the exact
    32-query scan"""
    if k > 48:
        return 0
    if form == "int8":
        return nq - (nq % 256 if 24 < nq % 256 <= 32 else 0)
    n = 0
    while nq - n > 64:
        n += min(128, nq - n)
    return n


def _pair(x, d=D):
    from clip_retrieval_amd.knn import Mi355xIndex
    from oracle.knn_oracle import FlatIPOracle

    o, ix = FlatIPOracle(d), Mi355xIndex(d)
    o.add(x)
    ix.add(x)
    return o, ix


def _counters(ix, form, s0, served, max_failed):
    s1 = (*ix.stats(), ix.i8_served())
    print(f"{form}: served {s1[0] - s0[0]} (want {served}), failed proofs {s1[1] - s0[1]}, int8 {s1[2] - s0[2]}")
    assert s1[0] - s0[0] == served, "the proof-based passes did not serve these batches"
    assert (s1[2] - s0[2] > 0) == (form == "int8"), "the wrong form of the pass served these batches"
    assert max_failed is None or s1[1] - s0[1] <= max_failed, f"{s1[1] - s0[1]} proofs failed"


@pytest.mark.parametrize("n,cases,max_failed", [
    (60_013, [(256, 40), (129, 1), (65, 48), (128, 64), (300, 40)], 8),  # ring revolutions, ragged tail, a second step of 44
    (4_097, [(200, 10)], 0), (4_112, [(200, 10)], 0), (4_113, [(200, 10), (32, 10)], 0),  # last unit of 1, 16, 16 + 1 rows; idle workgroups
    (33, [(65, 40)], None),  # fewer rows than J: thresholds of -inf (every row floods the staging lists), short answers
])
def test_parity(form, n, cases, max_failed):
    x = _data(n, D, seed=21)
    o, ix = _pair(x)
    s0 = (*ix.stats(), ix.i8_served())
    for nq, k in cases:
        q = _queries(nq, D, seed=nq + k, x=x)
        Dg, I = ix.search(q, k)
        Do, Io = o.search(q, k)
        _check(Dg, I, Do, Io, f"{form} n={n} nq={nq} k={k}")
        assert n >= k or ((I[:, n:] == -1).all() and (Dg[:, n:] == NEG).all())
    _counters(ix, form, s0, sum(_served(nq, k, form) for nq, k in cases), max_failed)
    ix.close()


def test_every_slab_and_row_position_reaches_the_product(form):
    """Query j is row r_j of x with every column outside slab j % 40 set to zero (32 columns left), scaled to unit length like every
    query of this suite; r_j walks the 32 positions of a tile (j % 32) over the first tile, a middle one and the ragged last one, row
    N - 1 included.  k = 1: the id must be r_j and D the float64 product.  A dropped, doubled or shifted fragment on either register
    file, or a row of the wrong half, changes an id or fails a proof.  (Unscaled, the own score is 0.025 +- 0.006 against a 9th best of
    0.013: the 0.01 margin below cannot hold for 160 queries at once; at unit length it is 0.16 against 0.08.  SEED is the first for
    which the float64 reference alone passes.)  Two calls of 96, so that the fp16 form's 128-query steps take every query."""
    n, SEED = 4_113, 0
    x = _data(n, D, seed=SEED)
    j = np.arange(160)
    r = np.minimum(np.array([0, 64, n // 32])[(j // 32) % 3] * 32 + j % 32, n - 1)
    r[-1] = n - 1
    q = np.zeros((160, D), np.float32)
    for i in j:
        s = slice(32 * (i % 40), 32 * (i % 40) + 32)
        q[i, s] = x[r[i], s].astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    s64 = np.sort(q.astype(np.float64) @ x.astype(np.float64).T, axis=1)
    assert (s64[:, -1] - s64[:, -9] > 0.01).all(), "test bug: the proof's margin (J = k + 8) is not certain on this seed"
    o, ix = _pair(x)
    s0 = (*ix.stats(), ix.i8_served())
    got = [ix.search(q[a:b], 1) for a, b in ((0, 96), (64, 160))]
    Dg, I = (np.concatenate([g[0][:64], g[1]]) for g in zip(*got))
    assert np.array_equal(got[0][1][64:], got[1][1][:32])
    assert np.array_equal(I[:, 0], r), np.argwhere(I[:, 0] != r)[:8].tolist()
    assert np.abs(Dg[:, 0].astype(np.float64) - s64[:, -1]).max() <= 1e-5
    _counters(ix, form, s0, 192, 0)
    ix.close()


def test_fallback_and_overflow(form):
    """300 rows tiled 20 times: every score exists 20 times, so the rows at the threshold (J = 48 falls into the third group of copies)
    tie exactly and ids must come back ascending among ties.  At this width the sample scores are exact and the fp16 threshold carries a
    slack of 1e-3 (as at d = 1024), so ties alone fail no proof; queries 0 .. 15 are the zero vector -- every row scores 0 = their
    threshold, 16 hits per query and unit flood their wave's 128-entry staging list -- and take the gated exact scans."""
    x = np.tile(_data(300, D, seed=12), (20, 1))
    q = _queries(256, D, seed=296, x=x)
    q[:16] = 0.0
    o, ix = _pair(x)
    s0 = (*ix.stats(), ix.i8_served())
    Dg, I = ix.search(q, 40)
    Do, Io = o.search(q, 40)
    assert np.array_equal(I, Io), "ids (ties in ascending id order)"
    assert np.allclose(Dg, Do, rtol=0, atol=1e-5)
    _counters(ix, form, s0, 256, None)
    if form == "fp16":
        assert ix.stats()[1] - s0[1] > 0, "expected failed proofs (the fallback is untested otherwise)"
    ix.close()


def test_padded_width_and_partial_copy(form, monkeypatch):
    """User width 1152 (padded to 1280; its zero pad columns make the int8 stage take two planes) with an int8 copy of half the rows:
    the int8 part and the fp16 rest (row_off) write one hit list; neighbours planted on both sides of the boundary."""
    d, n = 1152, 40_000
    monkeypatch.setenv("KNNX_I8_MAX_BYTES", str(20_000 * D))
    n8 = 20_000 // 32 * 32
    x = _data(n, d, seed=61)
    o, ix = _pair(x, d)
    rows = np.r_[0, 17, n8 - 1, n8, n8 + 1, n8 + 33, n - 1, n - 2, np.random.default_rng(62).integers(0, n, 192)]
    q = x[rows].astype(np.float32) + 0.02 * np.random.default_rng(63).standard_normal((200, d)).astype(np.float32)
    s0 = (*ix.stats(), ix.i8_served())
    Dg, I = ix.search(q, 10)
    Do, Io = o.search(q, 10)
    _check(Dg, I, Do, Io, f"{form} padded width, partial copy")
    assert np.array_equal(I[:8, 0], rows[:8])
    assert ix.i8_rows() == (n8 if form == "int8" else 0)
    _counters(ix, form, s0, 200, 0)
    ix.close()
