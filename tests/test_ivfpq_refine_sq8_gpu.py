"""The SQ8 refine store of IVF-PQ (faiss ",Refine(SQ8)") on the GPU against the numpy restatement of the SQ8 contract (knnx.h) below."""
import os

import numpy as np
import pytest

from build_cases import CHUNK, D, M, N, NLIST, corpus, fill_rows
from clip_retrieval_amd import knn
from oracle.knn_oracle import synth_mixture_rows
from test_ivfpq_gpu import _data, _queries, _seed_codebooks
from test_ivfpq_refine_gpu import _lists_of

pytestmark = pytest.mark.gpu
F32 = np.float32


def np_ranges(x):
    return x.astype(F32).min(0), x.astype(F32).max(0) - x.astype(F32).min(0)


def np_dec_enc(x, vmin, vdiff):
    """code = clamp((int)((x - vmin) * (255 / vdiff)), 0, 255), dec = vmin + (code + 0.5) * (vdiff / 255), each operation rounded to fp32"""
    code = np.clip(np.trunc((x.astype(F32) - vmin) * (F32(255) / vdiff)), 0, 255).astype(np.uint8)
    return vmin + (code.astype(F32) + F32(0.5)) * (vdiff / F32(255)), code


def _build(route, emb=None, **over):
    c = corpus()  # (the ranges are those of the first half of the rows, so the rest clamps)
    kw = {**dict(nprobe=4, centroids=c["cent"], codebooks=c["codebooks"], refine="sq8", refine_ranges=np_ranges(c["x"][:N // 2]), k_factor=8,
                 chunk=CHUNK), **over}
    if route == "folder":
        return knn.build_ivfpq_index_from_folder(emb, NLIST, M, **kw)
    if route == "device":
        return knn.build_ivfpq_index_device(fill_rows, N, D, NLIST, M, **kw)[0]
    return knn.build_ivfpq_index(c["x"], NLIST, M, **kw)


@pytest.fixture(scope="module")
def sq8():
    ix = _build("array")
    yield ix
    ix.close()


@pytest.mark.parametrize("d", [256, 512, 768, 1024])
def test_score_parity(d):
    """D against float64 <q, dec(code)>, I against the float64 ranking of the same candidates (those of the plain index at k = kc), at
    the 16-lane, 32-lane, ragged 48-lane and full-wave forms; kc = 510 (k = 10: the most it can ask for) and 512 (k = 64).
    Tolerance per score: gamma * sum_c |q_c dec_c|, gamma = (d / 64 + 8) * 2^-24: d / 64 for a lane's chain, 6 for the deepest butterfly,
    2 for the roundings of u = q * step and of b_q + sum.  (The kernel's chains are 16 long at every width, so below d = 1024 this is
    tighter than the worst-case count 16 + log2(lanes) + 2.)  Ranks may differ from float64's only between candidates closer than twice
    that, in at most 1 % of the slots."""
    n, nlist, m = 2000, 16, 16
    x = _data(n, d, d)
    cent = x[np.random.default_rng(d + 1).choice(n, nlist, replace=False)]
    kw = dict(nprobe=nlist, centroids=cent, codebooks=_seed_codebooks(x, cent, _lists_of(x, cent), m, d + 2))
    q = _queries(5, d, d + 3, x)
    q[0] = x[17]          # a stored row
    q[1] = np.eye(d, dtype=F32)[d - 5]  # one column, in the last 16 (d = 768: lane 47's span)
    plain = knn.build_ivfpq_index(x, nlist, m, threshold_scan=True, **kw)
    ix = knn.build_ivfpq_index(x, nlist, m, refine="sq8", refine_ranges=np_ranges(x), **kw)
    dec = np_dec_enc(x, *np_ranges(x))[0].astype(np.float64)
    slots, loose, worst = 0, 0, 0.0
    for k, kf in ((10, 51), (64, 8)):
        ix.k_factor = kf
        (D_, I), cand = ix.search(q, k), plain.search(q, k * kf)[1]
        for i, qi in enumerate(q.astype(np.float64)):
            c = cand[i][cand[i] >= 0]
            E, tol = dec[c] @ qi, (d / 64 + 8) * 2.0 ** -24 * np.abs(dec[c] * qi).sum(1)
            order, pos = np.lexsort((c, -E)), {int(v): j for j, v in enumerate(c)}
            for j in range(k):
                g, e = pos[int(I[i, j])], order[j]  # (KeyError: the id is no candidate)
                worst = max(worst, abs(D_[i, j] - E[g]) / tol[g])
                assert abs(D_[i, j] - E[g]) <= tol[g], (d, k, i, j, D_[i, j], E[g], tol[g])
                assert g == e or abs(E[g] - E[e]) < 2 * max(tol[g], tol[e]), (d, k, i, j)
                slots, loose = slots + 1, loose + (g != e)
    print(f"d={d}: worst |D - E| / tolerance = {worst:.3f}, {loose} of {slots} slots ranked inside the tolerance band")
    assert loose <= 0.01 * slots
    plain.close(), ix.close()


@pytest.mark.parametrize("rect", [False, True])
def test_store_and_reconstruct(rect, sq8):
    """reconstruct of EVERY id (each list's first tile and pad-adjacent last row among them) and of -1, and the R of a search, are the
    bytes of numpy's dec(enc(x)), also behind a rectangular rotation 256 -> 512; the arena holds one byte per column."""
    c, ix = corpus(), sq8
    x, rng = c["x"], np_ranges(c["x"][:N // 2])
    if rect:
        y = knn.rotate_rows(c["rect"], x)
        cent = y[np.random.default_rng(3).choice(N, NLIST, replace=False)]
        ix = _build("array", centroids=cent, codebooks=_seed_codebooks(y, cent, _lists_of(y, cent), M, 4), rotation=c["rect"])
    want = np_dec_enc(x, *rng)[0]
    got = ix.reconstruct_batch(np.append(np.arange(N), -1))
    assert got[:N].tobytes() == want.tobytes() and got[N].tobytes() == b"\xff" * (4 * D)
    _, I, R = ix.search_and_reconstruct(c["q"], 10)
    assert (I >= 0).all() and R.tobytes() == want[I].tobytes()
    assert ix.pq_arena_bytes()[1] == ix.pq_arena_bytes()[0] // M * D
    assert ix is sq8 or ix.close() is None


def test_independence_and_save_load(tmp_path, sq8):
    """A query alone (its lists split over up to nprobe workgroups) and in a batch of 7 (fewer shares each) gets the same bytes; host
    array, embeddings folder and rows produced on the device build one index; a saved and loaded index searches byte-equal."""
    c, emb = corpus(), str(tmp_path / "emb")
    for nprobe in (NLIST, 4):
        sq8.nprobe = nprobe
        D7, I7 = sq8.search(c["q"][:7], 10)
        alone = [sq8.search(c["q"][i:i + 1], 10) for i in range(7)]
        assert np.concatenate([a[0] for a in alone]).tobytes() == D7.tobytes() and np.concatenate([a[1] for a in alone]).tobytes() == I7.tobytes()
    os.makedirs(emb)
    np.save(os.path.join(emb, "img_emb_0.npy"), c["x"])
    want = [a.tobytes() for a in sq8.search(c["q"], 10)]
    for route in ("folder", "device", "saved"):
        ix = knn.load_index(str(tmp_path / "saved")) if route == "saved" else _build(route, emb)
        assert ix.pq_refine_kind == "sq8" and not ix.pq_refine and ix.k_factor == 8 and [a.tobytes() for a in ix.search(c["q"], 10)] == want, route
        if route == "folder":
            knn.save_index(ix, str(tmp_path / "saved"))
        ix.close()


REFUSED = {  # (ix: the sq8 index; new: an empty index with a PQ quantizer; c: the corpus) -> the code the call answers with
    "append": (-5, lambda ix, new, c: ix.ivf_append(c["x"][:40])),
    "remove": (-5, lambda ix, new, c: ix.ivf_remove(np.arange(5))),
    "merge": (-5, lambda ix, new, c: ix.merge_from(new)),
    "merge_other": (-5, lambda ix, new, c: new.merge_from(ix)),
    "sharded": (-5, lambda ix, new, c: knn.ShardedMi355xIndex.from_shards([ix], [0])),
    "threshold": (-5, lambda ix, new, c: setattr(ix, "pq_threshold_scan", True)),
    "filtered": (-5, lambda ix, new, c: ix.search_filtered(c["q"][:1], 10, dedup_thr=0.9)),
    "fp16_after_sq8": (-4, lambda ix, new, c: (new.set_pq_refine_sq8(*c["ranges"]), new.set_pq_refine())),
    "sq8_after_fp16": (-4, lambda ix, new, c: (new.set_pq_refine(), new.set_pq_refine_sq8(*c["ranges"]))),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals(what, sq8):
    """Each follow-up answers KNNX_E_UNSUPPORTED (-5), a second kind of store on one index KNNX_E_STATE (-4); both name the store."""
    (code, call), new = REFUSED[what], knn.Mi355xIndex(D)
    new.set_pq_quantizer(M, corpus()["codebooks"])
    with pytest.raises(knn.HipLibraryError, match=rf"code {code}.*sq8 refine store"):
        call(sq8, new, corpus())
    new.close()
    assert sq8.ntotal == N and not sq8.pq_threshold_scan


def test_recall_next_to_the_fp16_store():
    """Recall@10 against brute force on test_refine_recall's corpus, k_factor 8: the sq8 store may fall below the fp16 store by no more
    than the share of candidate pairs whose exact scores are closer than the SQ8 error bound sum_c |q_c| step_c / 2."""
    n, d, nlist, m, k, kf = 6000, 512, 16, 32, 10, 8
    x = synth_mixture_rows(np.arange(n), d, 7, 40)
    cent, cb = knn.train_ivfpq(x, nlist, m, niter=4, pq_niter=6, seed=0)[:2]
    kw = dict(nprobe=nlist, centroids=cent, codebooks=cb)
    q, x32 = _queries(64, d, 8, x), x.astype(F32)
    exact = np.argsort(-(q @ x32.T), axis=1)[:, :k]
    got = {}
    for name, extra in (("fp16", dict(refine=True, k_factor=kf)), ("cand", dict(threshold_scan=True)), ("sq8", dict(refine="sq8", k_factor=kf))):
        ix = knn.build_ivfpq_index(x, nlist, m, **kw, **extra)
        got[name] = ix.search(q, k * kf if name == "cand" else k)[1]
        step = ix.pq_refine_ranges()[1] / F32(255) if name == "sq8" else None
        ix.close()
    recall = {s: float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(got[s], exact)])) for s in ("fp16", "sq8")}
    close = pairs = 0
    for qi, c in zip(q.astype(np.float64), got["cand"]):
        s = x32[c].astype(np.float64) @ qi
        gap = np.abs(s[:, None] - s[None, :])[np.triu_indices(len(s), 1)]
        close, pairs = close + int((gap < np.abs(qi) @ step / 2).sum()), pairs + gap.size
    print(f"recall@10 at k_factor {kf}: fp16 store {recall['fp16']:.4f}, sq8 store {recall['sq8']:.4f}; share of close candidate pairs {close / pairs:.4f}")
    assert recall["sq8"] >= recall["fp16"] - close / pairs, (recall, close / pairs)
