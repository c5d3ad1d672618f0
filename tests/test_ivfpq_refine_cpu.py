"""The refine store of IVF-PQ (faiss IndexRefineFlat(IndexIVFPQ)) without a device: the numpy restatement that the GPU tests compare
against (test_ivfpq_refine_gpu.py imports it from here), its own sanity, and the rules of the saved manifest."""
import json
import os

import numpy as np
import pytest

from oracle.knn_oracle import IVFFlatOracle, topk_sets_equal
from test_ivfpq_gpu import NEG, _data, _queries, _seed_codebooks, np_adc_search, np_encode

TOL = 1e-5  # device fp32 against float64, ADC and exact scores alike (the bound of test_ivfpq_gpu._check)


# ------------------------------------------------------------------------------------------------ numpy restatement
def np_refine_parts(q, x, cent, cb, codes, lists, id_base, nprobe, qc=None):
    """Per query: (ids of the rows of its probed lists, their ADC scores S, their exact scores E -- both float64), and the mask of
    queries whose probe set is ambiguous.  qc: the queries the candidate stage sees (A q behind a rotation); E is always q . f32(x)."""
    M, _, ds = cb.shape
    nlist = cent.shape[0]
    qc = q if qc is None else qc
    qd = qc.astype(np.float64)
    cs = qd @ cent.astype(np.float32).astype(np.float64).T
    lut = np.einsum("qmt,mjt->qmj", qd.reshape(q.shape[0], M, ds), cb.astype(np.float64))
    Eall = x.astype(np.float32).astype(np.float64) @ q.astype(np.float64).T  # [n, nq], once
    parts, amb = [], np.zeros(q.shape[0], dtype=bool)
    np_ = min(nprobe, nlist)
    for i in range(q.shape[0]):
        order = np.lexsort((np.arange(nlist), -cs[i]))
        if np_ < nlist and abs(cs[i, order[np_ - 1]] - cs[i, order[np_]]) <= 1e-6:
            amb[i] = True
        rows = np.flatnonzero(np.isin(lists, order[:np_]))
        S = cs[i, lists[rows]] + lut[i][np.arange(M)[None, :], codes[rows]].sum(1)
        E = Eall[rows, i]
        parts.append((rows + id_base, S, E))
    return parts, amb


def np_refine_search(parts, k, kc):
    """The strict restatement: candidates = top kc by (S descending, id ascending), result = their top k by (E descending, id ascending)."""
    n = len(parts)
    D = np.full((n, k), NEG, dtype=np.float64)
    I = np.full((n, k), -1, dtype=np.int64)
    for i, (ids, S, E) in enumerate(parts):
        cand = np.lexsort((ids, -S))[:kc]
        top = cand[np.lexsort((ids[cand], -E[cand]))[:k]]
        D[i, :len(top)] = E[top]
        I[i, :len(top)] = ids[top]
    return D, I


def check_refine(D, I, parts, amb, k, kc, ctx):
    """The parity check of a refine search against the restatement, with the candidate boundary as a band of TOL around the kc-th ADC
    score T: every returned id has S >= T - TOL, its D is within TOL of E, D does not increase, padding appears exactly when the
    probed lists hold fewer than k rows, and every row with S > T + TOL whose E exceeds the last returned score by more than TOL is
    returned."""
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == (len(parts), k) and I.shape == D.shape, ctx
    worst = 0.0
    for i, (ids, S, E) in enumerate(parts):
        if amb[i]:
            continue
        nv = min(k, len(ids))
        assert (I[i, :nv] >= 0).all() and (I[i, nv:] == -1).all(), f"{ctx}: query {i}: padding ({len(ids)} probed rows)"
        assert (D[i, nv:] == NEG).all(), f"{ctx}: query {i}: padding score"
        got = I[i, :nv]
        assert len(set(got.tolist())) == nv, f"{ctx}: query {i}: an id twice"
        where = {int(a): j for j, a in enumerate(ids)}
        assert all(int(a) in where for a in got), f"{ctx}: query {i}: an id outside the probed lists"
        at = np.array([where[int(a)] for a in got], dtype=np.int64)
        T = np.sort(S)[::-1][kc - 1] if len(ids) >= kc else -np.inf
        assert (S[at] >= T - TOL).all(), f"{ctx}: query {i}: a result below the candidate boundary by {(T - S[at]).max()}"
        err = np.abs(D[i, :nv].astype(np.float64) - E[at])
        worst = max(worst, err.max(initial=0))
        assert err.max(initial=0) <= TOL, f"{ctx}: query {i}: exact score off by {err.max()}"
        assert (np.diff(D[i, :nv]) <= 0).all(), f"{ctx}: query {i} not sorted"
        if nv:
            must = np.flatnonzero((S > T + TOL) & (E > float(D[i, nv - 1]) + TOL))
            missing = set(ids[must].tolist()) - set(got.tolist())
            assert not missing, f"{ctx}: query {i}: {len(missing)} sure candidates with a better exact score are missing"
    return worst


# ------------------------------------------------------------------------------------------------ the restatement's own sanity
def _cpu_index(n, d, nlist, M, seed):
    """A valid IVF-PQ index in numpy: random rows as centroids, float64 nearest-centroid lists, seeded codebooks, numpy codes."""
    x = _data(n, d, seed)
    cent = x[np.random.default_rng(seed + 1).choice(n, nlist, replace=False)]
    lists = (x.astype(np.float32) @ cent.astype(np.float32).T).argmax(1).astype(np.int32)
    cb = _seed_codebooks(x, cent, lists, M, seed + 2)
    codes, _ = np_encode(x.astype(np.float32) - cent[lists].astype(np.float32), cb)
    return x, cent, lists, cb, codes


def test_k_factor_1_gives_the_adc_ids():
    x, cent, lists, cb, codes = _cpu_index(1500, 64, 12, 16, 3)
    q = _queries(20, 64, 4, x)
    parts, amb = np_refine_parts(q, x, cent, cb, codes, lists, 7, 4)
    _, I = np_refine_search(parts, 10, 10)
    _, Io, ambo = np_adc_search(q, cent, cb, codes, lists, 7, 4, 10)
    assert np.array_equal(amb, ambo)
    assert np.array_equal(np.sort(I, axis=1), np.sort(Io, axis=1))
    # ... in the order of the exact scores
    D, _ = np_refine_search(parts, 10, 10)
    assert (np.diff(D, axis=1) <= 0).all()


def test_all_probed_rows_as_candidates_is_ivf_flat():
    x, cent, lists, cb, codes = _cpu_index(1500, 64, 12, 16, 5)
    q = _queries(20, 64, 6, x)
    for nprobe in (1, 4, 12):
        parts, _ = np_refine_parts(q, x, cent, cb, codes, lists, 0, nprobe)
        kc = max(len(p[0]) for p in parts)
        D, I = np_refine_search(parts, 10, kc)
        Do, Io = IVFFlatOracle(64, cent, lists, x).search(q, 10, nprobe)
        assert np.array_equal(I >= 0, Io >= 0)
        assert np.abs(D[I >= 0] - Do[I >= 0]).max() <= 2e-6
        assert not topk_sets_equal(I, D.astype(np.float32), Io, Do, tol=2e-6)


def test_check_accepts_the_restatement_and_rejects_a_wrong_answer():
    x, cent, lists, cb, codes = _cpu_index(1500, 64, 12, 16, 8)
    q = _queries(12, 64, 9, x)
    parts, amb = np_refine_parts(q, x, cent, cb, codes, lists, 0, 3)
    D, I = np_refine_search(parts, 10, 40)
    D32 = D.astype(np.float32)
    check_refine(D32, I, parts, amb, 10, 40, "restatement")
    Dp, Ip = np_refine_search(parts, 10, 10)  # k_factor 1 in the place of 4: a better candidate is missing somewhere
    if not np.array_equal(I, Ip):
        with pytest.raises(AssertionError):
            check_refine(Dp.astype(np.float32), Ip, parts, amb, 10, 40, "too few candidates")
    bad = D32.copy()
    bad[0, 0] += 1e-3
    with pytest.raises(AssertionError):
        check_refine(bad, I, parts, amb, 10, 40, "score off")


# ------------------------------------------------------------------------------------------------ the manifest rules
def _folder(tmp_path, man, with_emb=True):
    from clip_retrieval_amd import knn

    idx = tmp_path / "idx"
    idx.mkdir()
    emb = tmp_path / "emb"
    if with_emb:
        emb.mkdir()
        np.save(emb / "img_emb_0.npy", np.zeros((5, 256), np.float16))
        np.save(emb / "img_emb_1.npy", np.zeros((3, 256), np.float16))
    full = {"format": knn.IVFPQ_FORMAT, "d": 256, "nlist": 2, "M": 16, "nprobe": 1, "row_range": [0, 8]}
    full.update(man)
    (idx / knn.IVFPQ_MANIFEST).write_text(json.dumps(full))
    return knn, str(idx), str(emb), full


def test_manifest_without_the_flag_is_self_contained(tmp_path):
    knn, idx, _, man = _folder(tmp_path, {}, with_emb=False)
    assert knn.read_ivfpq_refine(idx, man) == (False, 1, None)
    with pytest.raises(ValueError, match="k_factor"):
        knn.read_ivfpq_refine(idx, dict(man, k_factor=4))


def test_manifest_flag_finds_the_embeddings(tmp_path):
    knn, idx, emb, man = _folder(tmp_path, {})
    files = knn.FolderRows(emb).manifest()
    man = dict(man, refine=True, k_factor=8, embeddings=files, embeddings_relative=os.path.relpath(emb, idx))
    on, kf, src = knn.read_ivfpq_refine(idx, man)
    assert on and kf == 8 and src.n == 8 and src.d == 256
    moved = dict(man, embeddings_relative="nowhere", embeddings=dict(files, folder="/nowhere"))
    with pytest.raises(FileNotFoundError, match="refine store.*needs the embeddings"):
        knn.read_ivfpq_refine(idx, moved)
    assert knn.read_ivfpq_refine(idx, moved, embeddings_folder=emb)[2].n == 8  # ... unless the caller names them
    for bad in (0, 513, 2.5, True, "8"):
        with pytest.raises(ValueError, match="k_factor"):
            knn.read_ivfpq_refine(idx, dict(man, k_factor=bad))
    with pytest.raises(ValueError, match="names no embeddings"):
        knn.read_ivfpq_refine(idx, {k: v for k, v in man.items() if k != "embeddings"})
    np.save(os.path.join(emb, "img_emb_1.npy"), np.zeros((4, 256), np.float16))  # a partition grew: ids no longer mean the same rows
    with pytest.raises(ValueError, match="embedding files changed"):
        knn.read_ivfpq_refine(idx, man)


def test_load_refuses_a_refine_folder_without_embeddings_before_touching_the_device(tmp_path):
    knn, idx, emb, man = _folder(tmp_path, {}, with_emb=False)
    man = dict(man, refine=True, k_factor=2, embeddings={"folder": emb, "files": [["img_emb_0.npy", 8]], "rows": 8, "d": 256},
               embeddings_relative="../emb")
    with open(os.path.join(idx, knn.IVFPQ_MANIFEST), "w", encoding="utf-8") as f:
        json.dump(man, f)
    np.save(os.path.join(idx, "ivf_pq_centroids.npy"), np.zeros((2, 256), np.float16))
    np.save(os.path.join(idx, "ivf_pq_codebooks.npy"), np.zeros((16, 256, 16), np.float32))
    np.save(os.path.join(idx, "ivf_pq_codes.npy"), np.zeros((8, 16), np.uint8))
    np.save(os.path.join(idx, "ivf_pq_lists.npy"), np.zeros(8, np.int32))
    with pytest.raises(FileNotFoundError, match="pass embeddings_folder="):
        knn.load_index(idx)
