"""IVF-SQ8 without a GPU: the numpy restatement of the quantiser (include/knnx.h, "IVF-SQ8") with its self-checks, the index-key
parser, the manifest, and the quality condition -- the restatement's top-10 against the exact top-10 on the project's own corpora.
The GPU tests (test_ivfsq_gpu.py) hold the kernels to this restatement."""
import numpy as np
import pytest

from oracle.knn_oracle import planted_queries, synth_mixture_rows, synth_rows

NEG = np.float32(-3.4028234663852886e38)
MIX_CLUSTERS = 40  # clusters of the mixture corpus (what the IVF-PQ training test uses at this size)


# ------------------------------------------------------------------------------------------------ numpy restatement
def np_ranges(x_f16):
    """(vmin, vdiff) f32 [d] of a training set: faiss RS_minmax with argument 0."""
    x = np.asarray(x_f16).astype(np.float32)
    vmin, vmax = x.min(0), x.max(0)
    return vmin, (vmax - vmin).astype(np.float32)


def np_scale_step(vdiff):
    """scale = 255 / vdiff (0 where vdiff == 0), step = vdiff / 255, both in float32 with IEEE division."""
    vdiff = np.asarray(vdiff, dtype=np.float32)
    with np.errstate(divide="ignore"):
        scale = np.where(vdiff == 0, np.float32(0), np.float32(255) / vdiff).astype(np.float32)
    return scale, (vdiff / np.float32(255)).astype(np.float32)


def np_sq_encode(x_f16, vmin, vdiff):
    """u8 [n, d]: clip(floor((f32(x) - vmin) * scale), 0, 255), the subtract and the multiply each rounded to float32."""
    scale, _ = np_scale_step(vdiff)
    t = ((np.asarray(x_f16).astype(np.float32) - np.asarray(vmin, dtype=np.float32)).astype(np.float32) * scale).astype(np.float32)
    return np.clip(np.floor(t), 0, 255).astype(np.uint8)


def np_sq_decode(codes, vmin, vdiff):
    """f32 [n, d]: vmin + (f32(code) + 0.5) * step, the multiply and the add each rounded to float32."""
    _, step = np_scale_step(vdiff)
    p = ((codes.astype(np.float32) + np.float32(0.5)) * step).astype(np.float32)
    return (np.asarray(vmin, dtype=np.float32) + p).astype(np.float32)


def np_sq_scores(q, codes, vmin, vdiff):
    """float64 [nq, n]: <q, dec(row)> from the float32 decoded rows."""
    return q.astype(np.float64) @ np_sq_decode(codes, vmin, vdiff).astype(np.float64).T


def np_sq_search(q, cent, codes, lists, vmin, vdiff, id_base, nprobe, k):
    """D (float64), I of faiss IndexIVFScalarQuantizer.search on these codes, plus a mask of queries whose probe set is ambiguous (the
    nprobe-th and the next coarse score within 1e-6).  Order: score descending, ties by ascending id; -1 / -FLT_MAX padding."""
    nlist = cent.shape[0]
    qd = q.astype(np.float64)
    cs = qd @ cent.astype(np.float32).astype(np.float64).T
    s_all = np_sq_scores(q, codes, vmin, vdiff)
    n = q.shape[0]
    D = np.full((n, k), NEG, dtype=np.float64)
    I = np.full((n, k), -1, dtype=np.int64)
    amb = np.zeros(n, dtype=bool)
    np_ = min(nprobe, nlist)
    for i in range(n):
        order = np.lexsort((np.arange(nlist), -cs[i]))
        if np_ < nlist and abs(cs[i, order[np_ - 1]] - cs[i, order[np_]]) <= 1e-6:
            amb[i] = True
        rows = np.flatnonzero(np.isin(lists, order[:np_]))
        s = s_all[i, rows]
        top = np.lexsort((rows, -s))[:k]
        D[i, :len(top)] = s[top]
        I[i, :len(top)] = rows[top] + id_base
    return D, I, amb


def np_layout_old_to_new(lists, nlist):
    """old_to_new of rows added in id order with every row taking the next free position of its list: id i -> dense0[list] + rank."""
    lists = np.asarray(lists)
    order = np.argsort(lists, kind="stable")  # the rows list by list, ascending id inside a list = new_to_old
    o2n = np.empty(lists.shape[0], dtype=np.int64)
    o2n[order] = np.arange(lists.shape[0])
    return o2n


def corpus(kind, d, n):
    return synth_rows(np.arange(n), d, 7) if kind == "isotropic" else synth_mixture_rows(np.arange(n), d, 7, MIX_CLUSTERS)


def top10_overlap(exact_scores, approx_scores):
    a = np.argsort(-exact_scores, axis=1, kind="stable")[:, :10]
    b = np.argsort(-approx_scores, axis=1, kind="stable")[:, :10]
    return float(np.mean([len(set(x) & set(y)) / 10 for x, y in zip(a.tolist(), b.tolist())]))


# ------------------------------------------------------------------------------------------------ restatement self-checks
def test_decode_of_encode_is_within_half_a_step_inside_the_range():
    rng = np.random.default_rng(0)
    x = (0.2 * rng.standard_normal((500, 256))).astype(np.float16)
    vmin, vdiff = np_ranges(x)
    assert (vdiff > 0).all()
    codes = np_sq_encode(x, vmin, vdiff)
    assert codes.dtype == np.uint8 and codes.min() == 0 and codes.max() >= 254  # the column minima and maxima themselves
    dec = np_sq_decode(codes, vmin, vdiff)
    _, step = np_scale_step(vdiff)
    err = np.abs(dec.astype(np.float64) - x.astype(np.float64))
    # half a step, plus the float32 roundings of t near a code boundary and of the decode (a few ulp of the range)
    assert (err <= 0.5 * step.astype(np.float64) + 8 * np.spacing(np.abs(vmin) + vdiff).astype(np.float64)).all()


def test_values_outside_the_range_are_clamped():
    vmin, vdiff = np.full(256, -0.125, np.float32), np.full(256, 0.25, np.float32)
    x = np.zeros((3, 256), np.float16)
    x[0], x[1], x[2] = -5.0, 5.0, 0.125  # below, above, the maximum itself (t = 255 exactly)
    codes = np_sq_encode(x, vmin, vdiff)
    assert (codes[0] == 0).all() and (codes[1] == 255).all() and (codes[2] == 255).all()
    dec = np_sq_decode(codes, vmin, vdiff)
    # (code 255 decodes to the middle of the last bin counted from t = 255: half a step ABOVE vmin + vdiff, as in faiss)
    assert (dec >= vmin).all() and (dec <= vmin + vdiff * np.float32(256 / 255)).all()


def test_constant_columns_give_code_zero_and_vmin_back():
    rng = np.random.default_rng(1)
    x = (0.1 * rng.standard_normal((64, 256))).astype(np.float16)
    x[:, 5] = np.float16(0.25)
    x[:, 200:] = 0  # zero padding
    vmin, vdiff = np_ranges(x)
    assert vdiff[5] == 0 and (vdiff[200:] == 0).all()
    scale, step = np_scale_step(vdiff)
    assert scale[5] == 0 and step[5] == 0 and np.isfinite(scale).all()
    codes = np_sq_encode(x, vmin, vdiff)
    assert (codes[:, 5] == 0).all() and (codes[:, 200:] == 0).all()
    dec = np_sq_decode(codes, vmin, vdiff)
    assert (dec[:, 5] == np.float32(np.float16(0.25))).all() and (dec[:, 200:] == 0).all()
    # a row outside the constant column's "range" still encodes to 0 there
    y = x[:2].copy()
    y[:, 5] = 3.0
    assert (np_sq_encode(y, vmin, vdiff)[:, 5] == 0).all()


def test_score_is_bias_plus_weighted_codes():
    """The form the scan evaluates -- b_q + sum_j u_j code_j, u = q * step, b_q = <q, vmin + step / 2> -- is <q, dec(row)>: in float32
    within 7e-7 of the float64 value on unit-norm data."""
    x = corpus("isotropic", 768, 500)
    vmin, vdiff = np_ranges(x)
    codes = np_sq_encode(x, vmin, vdiff)
    _, step = np_scale_step(vdiff)
    q = planted_queries(np.arange(0, 500, 50), 768, 7)
    want = np_sq_scores(q, codes, vmin, vdiff)
    u = (q * step).astype(np.float32)
    bq = (q.astype(np.float64) @ (vmin.astype(np.float64) + 0.5 * step.astype(np.float64))).astype(np.float32)
    got = (u @ codes.astype(np.float32).T + bq[:, None]).astype(np.float32)
    assert np.abs(got.astype(np.float64) - want).max() <= 7e-7


def test_layout_restatement():
    lists = np.array([2, 0, 2, 1, 0, 2], dtype=np.int32)
    assert np_layout_old_to_new(lists, 3).tolist() == [3, 0, 4, 2, 1, 5]


# ------------------------------------------------------------------------------------------------ index key, manifest
def test_index_key_parser():
    from clip_retrieval_amd.knn import ivfsq_params_from_index_key

    assert ivfsq_params_from_index_key("IVF4096,SQ8") == {"nlist": 4096}
    assert ivfsq_params_from_index_key("IVF65536_HNSW32,SQ8") == {"nlist": 65536}
    assert ivfsq_params_from_index_key(" IVF24 , SQ8 ") == {"nlist": 24}
    for key, part in (("IVF4096,SQ4", "SQ4"), ("IVF4096,SQ6", "SQ6"), ("IVF4096,SQfp16", "SQfp16"), ("IVF4096", ""),
                      ("IVF0,SQ8", "IVF0"), ("Flat", "Flat"), ("OPQ64,IVF4096,SQ8", "OPQ64"), ("IVF4096,SQ8,RFlat", "RFlat"),
                      ("IVF4096,PQ64x8", "PQ64x8"), ("", "")):
        with pytest.raises(ValueError, match=f"index key part '{part}'"):
            ivfsq_params_from_index_key(key)


def test_manifest_round_trip(tmp_path):
    import json

    from clip_retrieval_amd import knn

    man = knn.ivfsq_manifest(768, 4096, 16, (1000, 7000))
    assert man["kind"] == "ivfsq" and man["format"] == knn.IVFSQ_FORMAT
    p = tmp_path / knn.IVFSQ_MANIFEST
    p.write_text(json.dumps(man), encoding="utf-8")
    back = knn.check_ivfsq_manifest(json.loads(p.read_text(encoding="utf-8")), str(p))
    assert back == man and back["row_range"] == [1000, 7000] and back["nprobe"] == 16
    for bad in ({**man, "kind": "ivfpq"}, {**man, "format": knn.IVFPQ_FORMAT}, {**man, "row_range": [5, 1]}, {**man, "nlist": 0}):
        with pytest.raises(ValueError):
            knn.check_ivfsq_manifest(bad, "x")
    # the three folder kinds are told apart by their manifest file
    assert len({knn.IVF_MANIFEST, knn.IVFPQ_MANIFEST, knn.IVFSQ_MANIFEST}) == 3
    assert knn.IVFSQ_MANIFEST.startswith("ivf_")  # (an index saved into its embeddings folder adds no partition: embedding_files)


# ------------------------------------------------------------------------------------------------ quality condition
@pytest.mark.parametrize("kind", ["isotropic", "mixture"])
@pytest.mark.parametrize("d,n", [(256, 6000), (768, 6000), (1024, 4000)])
def test_sq8_ranking_is_practically_the_exact_one(kind, d, n):
    """Mean overlap of the SQ8 top-10 with the exact top-10 over all rows >= 0.95 (measured with this restatement: 0.983 .. 0.989);
    64 planted queries on evenly spaced rows, ranges from the corpus itself."""
    x = corpus(kind, d, n)
    vmin, vdiff = np_ranges(x)
    codes = np_sq_encode(x, vmin, vdiff)
    rows = np.linspace(0, n - 1, 64).astype(np.int64)
    if kind == "isotropic":
        q = planted_queries(rows, d, 7)
    else:  # the same recipe on the mixture corpus: the row plus noise, normalised
        rng = np.random.default_rng(4)
        q = x[rows].astype(np.float32) + 0.1 * rng.standard_normal((64, d)).astype(np.float32) / np.sqrt(np.float32(d))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    exact = q.astype(np.float64) @ x.astype(np.float64).T
    approx = np_sq_scores(q, codes, vmin, vdiff)
    ov = top10_overlap(exact, approx)
    err = np.abs(approx - exact)
    print(f"{kind} d={d} n={n}: overlap {ov:.4f}, max score error {err.max():.2e}, rms {np.sqrt((err ** 2).mean()):.2e}")
    assert ov >= 0.95
