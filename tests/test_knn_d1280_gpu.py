"""kNN at width 1280 (ViT-bigG/14 embeddings): the scan whose lo fragments are split between the LDS and registers, and the kernels around
it, against float64 numpy on the same fp16 rows and f32 queries.  D is held to the 1e-5 of tests/test_knn_gpu.py's flat parity test and
ids must be EQUAL, so the inputs must not ask for an order that fp32 cannot give: every reference first asserts that no two neighbouring
scores of its own top k + 1 lie within TIE, and the data seeds (the last parameter of a case) are the first ones for which the float64
reference alone says so.  TIE: a score here is 160 fp32 accumulations of partial sums below 0.13 in magnitude (the rows that are not the
query's own source), each rounding by at most 2^-25 x 0.13 = 4e-9: 5e-8 as a random walk over the 160 steps, and TIE is five times that; the hi / lo split
of the query adds at most 2^-22 x sum |x q| < 1e-8."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_knn_gpu import NEG, _data, _queries

pytestmark = pytest.mark.gpu
D = 1280
TIE = 2.5e-7


def _ref(x, q, k, allowed=None):
    """(D, I) [nq, k] of the float64 scores by (score desc, id asc); allowed [nq, n]: the candidate rows of every query"""
    s = q.astype(np.float64) @ x.astype(np.float64).T
    s = s if allowed is None else np.where(allowed, s, -np.inf)
    o = np.argsort(-s, axis=1, kind="stable")[:, :k + 1]
    t = np.take_along_axis(s, o, 1)
    assert not (np.abs(np.diff(t, axis=1))[np.isfinite(t[:, 1:])] < TIE).any(), "test bug: a near-tie among the reference's top k + 1"
    m = min(k, o.shape[1])
    Dr, Ir, ok = np.full((len(q), k), NEG, np.float32), np.full((len(q), k), -1, np.int64), np.isfinite(t[:, :m])
    Dr[:, :m][ok], Ir[:, :m][ok] = t[:, :m][ok], o[:, :m][ok]
    return Dr, Ir


def _same(got, want, ctx):
    assert np.array_equal(got[1], want[1]), f"{ctx}: ids differ at {np.argwhere(got[1] != want[1])[:5].tolist()}"
    err = np.abs(got[0].astype(np.float64) - want[0]).max()
    print(f"{ctx}: max |D - D64| = {err:.3g}")
    assert err <= 1e-5, ctx


@pytest.mark.parametrize("n,nq,k,d,seed", [(1, 1, 1, D, 0), (33, 33, 40, D, 0), (4097, 33, 64, D, 12), (4097, 70, 40, D, 2), (4097, 3, 100, D, 0),
                                           (4097, 33, 40, 1152, 0)])
def test_flat_parity_and_reconstruct(n, nq, k, d, seed):
    """one row; a ragged second tile with short answers; k = 64 (the fast path's largest); three query groups; the large-k path; a user
    width padded to 1280.  search_and_reconstruct / reconstruct return the fp16 rows bit for bit, pad columns cut."""
    from clip_retrieval_amd.knn import Mi355xIndex

    x = _data(n, d, seed=seed)
    q = _queries(nq, d, seed=seed + 1, x=x)
    ix = Mi355xIndex(d)
    ix.add(x)
    _same(ix.search(q, k), _ref(x, q, k), f"flat n={n} nq={nq} k={k} d={d}")
    Dg, I, R = ix.search_and_reconstruct(q, min(k, n))
    assert R.shape == (nq, min(k, n), d) and np.array_equal(R, x[I].astype(np.float32))
    assert np.array_equal(ix.reconstruct(n - 1), x[n - 1].astype(np.float32))
    ix.close()


def test_operand_split_is_exact():
    """One-hot rows, q[c] = 0.5 + pi(c) 2^-23: every hi part is 0.5, every lo * 2048 part pi(c) 2^-12, every score exact in fp32.  A lo
    fragment dropped, doubled or shifted by a k-step on either side of the LDS / register boundary changes ids and bits."""
    from clip_retrieval_amd.knn import Mi355xIndex

    pi = np.random.default_rng(0).permutation(D)
    q = (np.float32(0.5) + pi.astype(np.float32) * np.float32(2.0**-23))[None]
    ix = Mi355xIndex(D)
    ix.add(np.eye(D, dtype=np.float16))
    want = np.argsort(-pi, kind="stable")[:64]
    Dg, I = ix.search(q, 64)
    assert np.array_equal(I[0], want) and Dg[0].tobytes() == q[0, want].tobytes()
    lims, Dr, Ir = ix.range_search(q, 0.5 + 1215.5 * 2.0**-23)
    assert lims.tolist() == [0, 64] and np.array_equal(np.sort(Ir), np.sort(want))
    ix.close()


@pytest.mark.parametrize("n,nlist,nprobe,seed", [(5000, 16, 16, 10), (5000, 16, 3, 3), (40, 8, 3, 0)])
def test_ivf_flat(n, nlist, nprobe, seed):
    """assignment = float64 argmax over the fp16 centroids (first maximum: the smaller list); search = the top-k of the rows of the
    probed lists (nprobe = nlist: of all rows); an append and a removal leave the index a fresh build answers bit for bit."""
    from clip_retrieval_amd.knn import build_ivf_index

    x = _data(n, D, seed=seed)
    cent = x[np.random.default_rng(seed).choice(n, nlist, replace=False)]
    ix = build_ivf_index(x, nlist, nprobe=nprobe, centroids=cent)
    c = np.sort(x.astype(np.float64) @ cent.astype(np.float64).T, axis=1)
    assert (c[:, -1] - c[:, -2] > TIE).all(), "test bug: a row between two centroids"
    assert np.array_equal(ix.ivf_lists, (x.astype(np.float64) @ cent.astype(np.float64).T).argmax(1))
    for nq, k in [(1, 40), (45, 64)]:
        q = _queries(nq, D, seed=seed + k, x=x)
        cs = q.astype(np.float64) @ cent.astype(np.float64).T
        assert np.abs(np.diff(np.sort(cs, axis=1), axis=1)).min() > TIE, "test bug: a query between two centroids"
        probes = np.argsort(-cs, axis=1, kind="stable")[:, :nprobe]
        allowed = (np.asarray(ix.ivf_lists)[None, :, None] == probes[:, None, :]).any(2)
        assert allowed.all() == (nprobe == nlist)
        _same(ix.search(q, k), _ref(x, q, k, allowed), f"ivf n={n} nprobe={nprobe} nq={nq} k={k}")
    if n == 5000 and nprobe == 3:
        rows, q = x, _queries(45, D, seed=9, x=x)
        for step in ("append", "remove"):
            if step == "append":
                ix.ivf_append(_data(300, D, seed=7))
                rows = np.concatenate([x, _data(300, D, seed=7)])
            else:
                rows = rows[ix.ivf_remove(np.arange(0, len(rows), 7))]
            fresh = build_ivf_index(rows, nlist, nprobe=nprobe, centroids=cent)
            for a, b in zip(ix.search_and_reconstruct(q, 10), fresh.search_and_reconstruct(q, 10)):
                assert a.tobytes() == b.tobytes(), step
            fresh.close()
    ix.close()


def test_search_dedup_and_search_filtered():
    """tests/test_filter_gpu.py's tile-edge corpus at width 1280 (160 orthonormal rows, 40 of them with a copy at similarity 0.97) through
    its restatement of the whole post filter, and the fused dedup's links against the same float64 statement."""
    from test_filter_gpu import THR, _check_request, _flat, _orthonormal, _prompts, _small_stack, _unit64

    rng = np.random.default_rng(21)
    basis = _orthonormal(rng, 240, D)
    rows = np.concatenate([basis[:160], 0.97 * basis[:40] + np.sqrt(1 - 0.97**2) * basis[160:200]]).astype(np.float16)
    ix = _flat(rows)
    q = rng.standard_normal(D).astype(np.float32)
    drop, stats = _check_request(ix, q, 200, _prompts(D, 22), _small_stack(D, 23))
    assert stats["n_valid"] == 200 and stats["n_links"] == 40
    Dg, I, R, links = ix.search_dedup(q[None], 64, THR, want_r=True)
    e = _unit64(rows[I[0]])
    assert np.array_equal(R[0], rows[I[0]].astype(np.float32))
    assert [tuple(p) for p in links.tolist()] == [(i, j) for i in range(64) for j in range(i + 1, 64) if e[i] @ e[j] > THR]
    ix.close()


def test_bigG_embeddings_reach_the_index_and_come_back():
    """inference -> index -> back at the widest model: the two-layer ViT-bigG/14-shaped encoder of tests/test_wide_heads_gpu.py, its image
    embeddings planted one at a time among random unit rows of Mi355xIndex(1280), found again by KnnHotPath.knn_search."""
    from clip_retrieval_amd.encoder import ClipEncoder, random_blob
    from clip_retrieval_amd.knn import Mi355xIndex
    from clip_retrieval_amd.service import KnnHotPath
    from oracle.clip_oracle import normalise_u8_nhwc, synth_pixels_u8
    from test_wide_heads_gpu import _oracle_arch, _product_arch

    parch = _product_arch(_oracle_arch("bigG"))
    enc = ClipEncoder(parch, random_blob(parch, 0), 0)
    emb = enc.encode_image(normalise_u8_nhwc(synth_pixels_u8(3, seed=3)))
    enc.close()
    assert emb.shape == (3, D) and emb.dtype == np.float16
    for j, row in enumerate((0, 250, 499)):
        x = _data(500, D, seed=1)
        x[row] = emb[j]
        ix = Mi355xIndex(D)
        ix.add(x)
        dist, ids = KnnHotPath().knn_search(emb[j:j + 1].astype(np.float32), "image", 40, SimpleNamespace(image_index=ix, text_index=ix),
                                            False, False, False)
        assert int(ids[0]) == row and float(dist[0]) > 0.999, (row, ids[:3], dist[:3])
        ix.close()
