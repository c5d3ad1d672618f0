"""The device post filter on the GPU: `Mi355xIndex.search_filtered` (knnx_search_filtered) against a numpy / scipy restatement in float64
over `index.reconstruct_batch(I)`, `KnnHotPath(device_filter=True)` against the general path, and knnx_mlp_forward_device against
knnx_mlp_forward.

Margins.  Every expectation first asserts, on the CPU, that its inputs keep every quantity away from its threshold: |sim - thr| > 1e-3 for
all pairs, |score - safety_thr| > 1e-3 (safety_thr: the midpoint of the widest gap among the sorted float64 scores in the middle half;
the head's last bias is shifted so that this threshold is the service's 0.5), |s1 - s0| > 1e-5 (unit prompts, reseeded by a fixed rule until the request's rows keep that distance).  That is 100 x the error bound of an fp32
chain at K <= 1024 (1.5e-7 x sum |a b|; sum |a b| <= 1 for unit rows, a few units for the heads used here).  Inputs that fail their own
margin are a bug of the test."""
import ctypes as C
import threading
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = 0.94


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def _unit64(rows):
    r = np.asarray(rows, dtype=np.float64)
    n = np.linalg.norm(r, axis=1)
    n[n == 0] = 1
    return r / n[:, None]


def _small_stack(d, seed):
    """A safety head small enough to be rebuilt per request: d -> 128 -> 16 -> 1, ReLU between, biases; the last layer is scaled so
    that the scores of unit rows spread over several units (the margin of 1e-3 is absolute)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for p, (i, o) in zip((0, 2, 4), ((d, 128), (128, 16), (16, 1))):
        sd[f"layers.{p}.weight"] = (rng.uniform(-1, 1, (o, i)) * np.sqrt(3.0 / i)).astype(np.float32)
        sd[f"layers.{p}.bias"] = (rng.uniform(-1, 1, o) * 0.1).astype(np.float32)
    sd["layers.0.weight"] *= np.float32(8.0)
    sd["layers.4.weight"] *= np.float32(40.0)
    return sd


def _stack64(sd, x):
    y = np.asarray(x, dtype=np.float64)
    pos = sorted(int(k.split(".")[1]) for k in sd if k.endswith(".weight"))
    for j, p in enumerate(pos):
        y = y @ sd[f"layers.{p}.weight"].astype(np.float64).T + sd[f"layers.{p}.bias"].astype(np.float64)
        if j + 1 < len(pos):
            y = np.maximum(y, 0)
    return y[:, 0]


def _safety_threshold(scores):
    s = np.sort(scores)
    lo, hi = len(s) // 4, len(s) - len(s) // 4
    if hi - lo < 2:
        return float(s[0]) - 0.5
    g = int(np.argmax(np.diff(s[lo:hi])))
    return float(0.5 * (s[lo + g] + s[lo + g + 1]))


def _pick_prompts(e, prompts):
    """`prompts`, or the first of a fixed sequence of reseeded prompt pairs whose two scores are more than 1e-5 apart for every row of this
    request (unit prompts over 3 000 unit rows put some row that close about one time in four).  A zero row is exempt: it scores exactly 0
    against every prompt in any arithmetic, and the first maximum is prompt 0."""
    live = np.any(e != 0, axis=1)
    for attempt in range(64):
        s = e[live] @ prompts.astype(np.float64).T
        if np.all(np.abs(s[:, 1] - s[:, 0]) > 1e-5):
            return prompts
        prompts = _prompts(prompts.shape[1], 1000 + attempt)
    raise AssertionError("test bug: no prompt pair without a violence near-tie")


def _expected(rows, k, prompts=None, sd=None, dedup=True):
    """(drop bytes [k], links, the safety state dict with its threshold moved to 0.5, the prompts used) from the reconstructed rows of the
    valid results."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    n = rows.shape[0]
    e = _unit64(rows)
    bits = np.zeros(k, np.uint8)
    n_links = 0
    if dedup and n:
        sim = e @ e.T
        iu = np.triu_indices(n, 1)
        assert np.all(np.abs(sim[iu] - THR) > 1e-3), "test bug: a pair within 1e-3 of the dedup threshold"
        link = np.triu(sim > THR, 1)
        n_links = int(link.sum())
        _, label = connected_components(csr_matrix(link), directed=False)
        first = np.full(label.max() + 1, n, dtype=np.int64)
        np.minimum.at(first, label, np.arange(n))
        bits[:n][first[label] != np.arange(n)] |= 1
    if prompts is not None and n:
        prompts = _pick_prompts(e, prompts)
        bits[:n][np.argmax(e @ prompts.astype(np.float64).T, axis=1) == 1] |= 2
    shifted = None
    if sd is not None and n:
        sc = _stack64(sd, e)
        thr = _safety_threshold(sc)
        assert np.all(np.abs(sc - thr) > 1e-3), "test bug: a safety score within 1e-3 of its threshold"
        shifted = dict(sd)
        shifted["layers.4.bias"] = (sd["layers.4.bias"].astype(np.float64) + (0.5 - thr)).astype(np.float32)
        sc = _stack64(shifted, e)  # (the shifted bias is an fp32 number: check the margin again where it counts)
        assert np.all(np.abs(sc - 0.5) > 1e-3)
        bits[:n][sc > 0.5] |= 4
    return bits, n_links, shifted, prompts


def _check_request(index, q, k, prompts, sd, hot_paths=None, dedup=True, use_v=True, use_s=True):
    """search_filtered == search + the restatement; optionally KnnHotPath switch on == switch off."""
    from clip_retrieval_amd.service import Mi355xSafetyHead

    q = np.ascontiguousarray(q, np.float32).reshape(1, -1)
    D0, I0 = index.search(q, k)
    n = int(np.argmax(I0[0] == -1)) if (I0[0] == -1).any() else k
    rows = index.reconstruct_batch(I0[0][:n]) if n else np.zeros((0, index.d), np.float32)
    want, n_links, shifted, prompts = _expected(rows, k, prompts if use_v else None, sd if use_s else None, dedup)
    vhead = Mi355xSafetyHead({"layers.0.weight": prompts}, relu=[False]) if use_v else None
    shead = Mi355xSafetyHead(shifted) if (use_s and shifted is not None) else None
    try:
        D, I, drop, stats = index.search_filtered(q, k, THR if dedup else None, vhead, shead, 0.5)
        assert np.array_equal(I, I0) and np.array_equal(D, D0)
        assert stats["n_valid"] == n and np.all(drop[n:] == 0)
        if dedup:
            assert stats["n_links"] == n_links and not stats["links_overflowed"]
            assert (stats["cc_rounds"] == 0) == (n_links == 0)
            assert stats["cc_rounds"] <= max(n, 1)
        assert np.array_equal(drop, want), (np.flatnonzero(drop != want)[:20], drop[drop != want][:20], want[drop != want][:20])
        if hot_paths is not None and shead is not None:
            res = SimpleNamespace(image_index=index, text_index=index, safety_model=shead, violence_detector=prompts)
            off = hot_paths[0].knn_search(q, "image", k, res, dedup, use_s, use_v)
            on = hot_paths[1].knn_search(q, "image", k, res, dedup, use_s, use_v)
            assert [int(i) for i in on[1]] == [int(i) for i in off[1]] and [float(x) for x in on[0]] == [float(x) for x in off[0]]
            sel = np.flatnonzero(want[:n] == 0)
            assert [int(i) for i in on[1]] == list(dict.fromkeys(int(i) for i in I0[0][:n][sel]))  # (ids are distinct here)
    finally:
        for h in (vhead, shead):
            if h is not None:
                h.close()
    return drop, stats


@pytest.fixture(scope="module")
def hot_paths():
    from clip_retrieval_amd.service import KnnHotPath

    return KnnHotPath(device_filter=False), KnnHotPath(device_filter=True)


def _prompts(d, seed):
    """Two unit rows, like the embeddings of the two prompts."""
    p = np.random.default_rng(seed).standard_normal((2, d))
    return (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)


def _orthonormal(rng, m, d):
    qm, _ = np.linalg.qr(rng.standard_normal((d, m)))
    return qm.T  # [m, d]


def _flat(rows):
    from clip_retrieval_amd.knn import Mi355xIndex

    ix = Mi355xIndex(rows.shape[1], coalesce=False)
    ix.add(np.ascontiguousarray(rows, np.float16))
    return ix


def _query_for_ranks(rows16, rank_of_row):
    """A query whose scores put row r at rank rank_of_row[r]: least squares over the stored (fp16) rows, scores 5e-3 apart."""
    target = 1.0 - 5e-3 * np.asarray(rank_of_row, dtype=np.float64)
    q, *_ = np.linalg.lstsq(rows16.astype(np.float64), target, rcond=None)
    q = q.astype(np.float32)
    got = np.argsort(-(rows16.astype(np.float64) @ q.astype(np.float64)), kind="stable")
    assert np.array_equal(np.asarray(rank_of_row)[got], np.arange(len(rank_of_row))), "test bug: the query does not give the ranks"
    return q


# ---- tile edges -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_index():
    """200 rows of width 256: 120 random unit rows and 40 pairs at similarity 0.97 whose members fall on either side of the 64-row
    tile edges once ranked."""
    rng = np.random.default_rng(21)
    d = 256
    basis = _orthonormal(rng, 240, d)
    rows = np.concatenate([basis[:160], 0.97 * basis[:40] + np.sqrt(1 - 0.97**2) * basis[160:200]])
    ix = _flat(rows)
    q = rng.standard_normal(d).astype(np.float32)
    yield ix, q, _prompts(d, 22), _small_stack(d, 23)
    ix.close()


@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 129, 200, 260])
def test_tile_edges_on_a_200_row_flat_index(edge_index, hot_paths, k):
    ix, q, prompts, sd = edge_index
    drop, stats = _check_request(ix, q, k, prompts, sd, hot_paths)
    assert stats["n_valid"] == min(k, 200)
    if k >= 200:
        assert stats["n_links"] == 40 and np.count_nonzero(drop & 1) == 40


# ---- link shapes ------------------------------------------------------------------------------------------------------------------
def _chain(rng, n, d, start=None, avoid=None):
    """x_{t+1} = normalize(0.96 x_t + 0.28 g_t), g_t fresh and orthogonal to everything before it: neighbours at 0.96, second
    neighbours at about 0.92."""
    basis = _orthonormal(rng, n + (0 if avoid is None else avoid.shape[0]), d)
    if avoid is not None:  # orthogonal to another family of rows as well
        basis = basis - (basis @ avoid.T) @ avoid
        basis = np.linalg.qr(basis.T)[0].T
    x = [basis[0] if start is None else start]
    for t in range(1, n):
        v = 0.96 * x[-1] + 0.28 * basis[t]
        x.append(v / np.linalg.norm(v))
    return np.stack(x)


@pytest.mark.parametrize("d", [256, 768])
def test_a_chain_is_one_group_whatever_the_ranks(d):
    """150 rows in a chain, transitive only; the result ranks are a random permutation along it, so the smallest label has to travel
    both ways."""
    rng = np.random.default_rng(31 + d)
    rows16 = _chain(rng, 150, d).astype(np.float16)
    rank = rng.permutation(150)
    ix = _flat(rows16)
    try:
        drop, stats = _check_request(ix, _query_for_ranks(rows16, rank), 150, _prompts(d, 32), _small_stack(d, 33))
        assert stats["n_links"] == 149 and np.count_nonzero(drop & 1) == 149 and not drop[0] & 1
        assert 2 <= stats["cc_rounds"] <= 150
    finally:
        ix.close()


@pytest.mark.parametrize("d", [256, 768])
def test_star_two_joined_chains_copies_and_a_zero_row(d):
    rng = np.random.default_rng(41 + d)
    basis = _orthonormal(rng, 200, d)
    # a star: the centre ranked LAST of its 30 leaves (leaf-leaf similarity 0.92: linked through the centre only)
    star = np.concatenate([0.96 * basis[0][None] + 0.28 * basis[1:31], basis[0][None]])
    # two chains of 40 joined by the one link between the members ranked last in each
    chains = _chain(rng, 80, d, avoid=basis[:62])
    # exact copies (5 of one row, 2 of another), a zero row, and rows that duplicate nothing
    singles = basis[40:60]
    rows = np.concatenate([star, chains, np.repeat(basis[60][None], 5, 0), np.repeat(basis[61][None], 2, 0), np.zeros((1, d)), singles])
    rows16 = rows.astype(np.float16)
    n = rows.shape[0]
    # ranks: the zero row must score 0 whatever the query, so it is ranked by a score of its own: everything else is placed around it
    zero = 31 + 80 + 7
    order = np.concatenate([np.arange(31), 31 + np.arange(40), 31 + 79 - np.arange(40), np.arange(31 + 80, n)])  # rows in rank order
    order = order[order != zero]
    rank = np.empty(n - 1, np.int64)
    live = np.delete(np.arange(n), zero)
    pos = {int(r): i for i, r in enumerate(order)}
    for j, r in enumerate(live):
        rank[j] = pos[int(r)]
    q = _query_for_ranks(rows16[live], rank)  # scores 1 .. 1 - 5e-3 (n - 2) > 0: the zero row (score 0) comes last
    ix = _flat(rows16)
    try:
        drop, stats = _check_request(ix, q, n + 5, _prompts(d, 42), _small_stack(d, 43))
        assert stats["n_valid"] == n
        # ranks: star leaves 0..29, centre 30 -> 30 dropped (everything but leaf 0); chains 31..110 -> 79 dropped; copies 4 + 1
        assert np.count_nonzero(drop & 1) == 30 + 79 + 5
        assert stats["n_links"] == 30 + 79 + 10 + 1
        assert not drop[n - 1] & 1  # the zero row, last: a duplicate of nothing
    finally:
        ix.close()


def test_no_duplicates_at_all_needs_no_component_rounds(hot_paths):
    rng = np.random.default_rng(51)
    d = 256
    ix = _flat(_orthonormal(rng, 130, d))
    try:
        drop, stats = _check_request(ix, rng.standard_normal(d).astype(np.float32), 130, _prompts(d, 52), _small_stack(d, 53), hot_paths)
        assert stats["n_links"] == 0 and stats["cc_rounds"] == 0 and not np.any(drop & 1)
        # dedup alone: nothing set at all
        drop, stats = _check_request(ix, rng.standard_normal(d).astype(np.float32), 130, None, None, use_v=False, use_s=False)
        assert not drop.any()
    finally:
        ix.close()


# ---- overflow ---------------------------------------------------------------------------------------------------------------------
def test_more_links_than_the_device_keeps(hot_paths):
    """1 600 copies of one row in a 3 000-row index at k = 3 000: 1.28 M links against the cap of 2^20."""
    from clip_retrieval_amd.service import Mi355xSafetyHead

    rng = np.random.default_rng(61)
    d, k = 256, 3000
    rows = rng.standard_normal((3000, d))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows[rng.permutation(3000)[:1600]] = rows[0]
    ix = _flat(rows)
    prompts, sd = _prompts(d, 62), _small_stack(d, 63)
    q = rng.standard_normal((1, d)).astype(np.float32)
    try:
        D0, I0 = ix.search(q, k)
        want, n_links, shifted, prompts = _expected(ix.reconstruct_batch(I0[0]), k, prompts, sd)
        assert n_links == 1600 * 1599 // 2 > 1 << 20
        vhead, shead = Mi355xSafetyHead({"layers.0.weight": prompts}, relu=[False]), Mi355xSafetyHead(shifted)
        D, I, drop, stats = ix.search_filtered(q, k, THR, vhead, shead, 0.5)
        assert np.array_equal(I, I0) and np.array_equal(D, D0)
        assert stats["links_overflowed"] == 1 and stats["n_links"] == n_links and stats["cc_rounds"] == 0
        assert not np.any(drop & 1) and np.array_equal(drop, want & 6)  # no duplicate bit at all, the other two still right
        res = SimpleNamespace(image_index=ix, text_index=ix, safety_model=shead, violence_detector=prompts)
        off = hot_paths[0].knn_search(q, "image", k, res, True, True, True)
        on = hot_paths[1].knn_search(q, "image", k, res, True, True, True)
        assert [int(i) for i in on[1]] == [int(i) for i in off[1]] and [float(x) for x in on[0]] == [float(x) for x in off[0]]
        assert [int(i) for i in on[1]] == [int(i) for i in I0[0][want == 0]]
        vhead.close(), shead.close()
    finally:
        ix.close()


# ---- every kind of index ------------------------------------------------------------------------------------------------------------
def _corpus(d):
    """6 000 fp16 rows: 4 000 random unit rows, then 2 000 EXACT copies (four each of rows 0, 3, 6, ...): a compressed index decodes
    copies to the same bits, so every similarity stays at 1 or far below the threshold whatever the codec does."""
    rng = np.random.default_rng(70 + d)
    base = rng.standard_normal((4000, d))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    x = np.concatenate([base, base[(np.arange(2000) % 500) * 3]]).astype(np.float16)
    q = (x[3].astype(np.float32) + 0.05 * rng.standard_normal(d).astype(np.float32))[None]
    return x, q


KINDS = ["flat", "ivf", "ivfsq", "ivfpq_opq", "ivfpq_refine"]


def _build(kind, x):
    from clip_retrieval_amd import knn

    if kind == "flat":
        return _flat(x)
    if kind == "ivf":
        return knn.build_ivf_index(x, 16, nprobe=12, niter=2)
    if kind == "ivfsq":
        return knn.build_ivfsq_index(x, 16, nprobe=12, niter=2, threshold_scan=True)
    if kind == "ivfpq_opq":
        return knn.build_ivfpq_index(x, 16, 16, nprobe=12, niter=2, pq_niter=2, opq=True, threshold_scan=True)
    return knn.build_ivfpq_index(x, 16, 16, nprobe=12, niter=2, pq_niter=2, refine=True, k_factor=2, threshold_scan=True)


@pytest.mark.parametrize("d", [256, 768])
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_of_index(hot_paths, kind, d):
    x, q = _corpus(d)
    ix = _build(kind, x)
    prompts, sd = _prompts(d, 71), _small_stack(d, 72)
    try:
        for k in (40, 100, 3000):
            drop, stats = _check_request(ix, q, k, prompts, sd, hot_paths)
            assert stats["n_valid"] == k
            assert np.count_nonzero(drop & 1) >= 4 and 0 < np.count_nonzero(drop & 2) < k and 0 < np.count_nonzero(drop & 4) < k
    finally:
        ix.close()


def test_ivfpq_without_its_threshold_scan_keeps_its_refusal():
    from clip_retrieval_amd import HipLibraryError, knn
    from clip_retrieval_amd.service import Mi355xSafetyHead

    x, q = _corpus(256)
    ix = knn.build_ivfpq_index(x[:2000], 8, 16, nprobe=8, niter=2, pq_niter=2)
    vhead = Mi355xSafetyHead({"layers.0.weight": _prompts(256, 71)}, relu=[False])
    try:
        with pytest.raises(HipLibraryError, match="k > 64 is not supported on an IVF-PQ index"):
            ix.search(q, 100)
        with pytest.raises(HipLibraryError, match="k > 64 is not supported on an IVF-PQ index"):
            ix.search_filtered(q, 100, THR, vhead, None)
        D, I, drop, stats = ix.search_filtered(q, 40, THR, vhead, None)  # k <= 64 is served as ever
        D0, I0 = ix.search(q, 40)
        assert np.array_equal(I, I0) and np.array_equal(D, D0) and stats["n_valid"] == 40
    finally:
        vhead.close()
        ix.close()


# ---- knnx_mlp_forward_device ------------------------------------------------------------------------------------------------------
def _h14_state_dict(seed=0, input_size=1024):
    """The seeded H14-shaped stack of tests/test_service_gpu.py (h14_nsfw_model.py:16-34)."""
    rng = np.random.default_rng(seed)
    widths = [input_size, 1024, 2048, 1024, 256, 128, 16, 1]
    positions = [0, 3, 6, 9, 12, 15, 16]
    sd = {}
    for p, (i, o) in zip(positions, zip(widths[:-1], widths[1:])):
        sd[f"layers.{p}.weight"] = (rng.uniform(-1, 1, (o, i)) * np.sqrt(3.0 / i)).astype(np.float32)
        sd[f"layers.{p}.bias"] = (rng.uniform(-1, 1, o) * 0.1).astype(np.float32)
    return sd


@pytest.mark.parametrize("width", [1024, 768])
def test_mlp_forward_device_equals_mlp_forward_bit_for_bit(lib, width):
    """Rows already on the device with row stride 1 024 (a 1 024-wide and a 768-wide input) -> the bits of knnx_mlp_forward."""
    import torch

    from clip_retrieval_amd._lib import check
    from clip_retrieval_amd.service import Mi355xSafetyHead

    head = Mi355xSafetyHead(_h14_state_dict(seed=5, input_size=width))
    assert head.device == 0 and lib.knnx_mlp_device(head._h) == 0  # pylint: disable=protected-access
    rng = np.random.default_rng(6)
    ld = 1024
    try:
        for n in (1, 63, 64, 65, 3000):
            padded = rng.standard_normal((n, ld)).astype(np.float32)  # (the columns past `width` are junk the layers must not read)
            x = np.ascontiguousarray(padded[:, :width])
            want = head.predict(x)
            xd = torch.from_numpy(padded).cuda()
            yd = torch.full((n, 1), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            check(lib, lib.knnx_mlp_forward_device(head._h, C.c_void_p(xd.data_ptr()), ld, n, C.c_void_p(yd.data_ptr()), None), "knnx")  # pylint: disable=protected-access
            got = yd.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), n
        rc = lib.knnx_mlp_forward_device(head._h, C.c_void_p(xd.data_ptr()), width - 1, 1, C.c_void_p(yd.data_ptr()), None)  # pylint: disable=protected-access
        assert rc == -1 and b"row stride" in lib.knnx_last_error()
    finally:
        head.close()


def test_mlp_handles_come_and_go_and_the_activations_regrow():
    """Twenty heads created and destroyed in a row; then on one handle knnx_mlp_forward at n = 1, at n = 5 000 -- past the 4 096 rows
    the activation buffers start with, so both are replaced -- and at n = 1 again.  Unit rows through the small stack: each result
    within 1e-3 of the float64 restatement (the margin every expectation of this file keeps, 100 x the fp32 chain's error bound), the
    two single rows the same bits."""
    from clip_retrieval_amd.service import Mi355xSafetyHead

    d = 256
    sd = _small_stack(d, 91)
    for _ in range(20):
        Mi355xSafetyHead(sd).close()
    x = _unit64(np.random.default_rng(92).standard_normal((5000, d))).astype(np.float32)
    want = _stack64(sd, x)
    head = Mi355xSafetyHead(sd)
    try:
        first, grown, again = head.predict(x[:1]), head.predict(x), head.predict(x[:1])
    finally:
        head.close()
    for got, n in ((first, 1), (grown, 5000), (again, 1)):
        assert got.shape == (n, 1)
        err = np.abs(got[:, 0].astype(np.float64) - want[:n]).max()
        assert err <= 1e-3, f"n = {n}: {err} from the float64 restatement"
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))


# ---- refusals and concurrency -----------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(edge_index):
    """k = 8193, a head of the wrong width, no filter, and (where the machine has a second GPU) a head on another device: each is refused,
    and a k = 40 answer read before and after is identical."""
    import torch

    from clip_retrieval_amd import HipLibraryError
    from clip_retrieval_amd.service import Mi355xSafetyHead

    ix, q, prompts, _ = edge_index
    q = q[None]
    vhead = Mi355xSafetyHead({"layers.0.weight": prompts}, relu=[False])
    narrow = Mi355xSafetyHead({"layers.0.weight": prompts[:, :128].copy()}, relu=[False])
    biased = Mi355xSafetyHead({"layers.0.weight": prompts, "layers.0.bias": np.ones(2, np.float32)}, relu=[False])
    try:
        before = ix.search_filtered(q, 40, THR, vhead, None)
        with pytest.raises(HipLibraryError, match="8192"):
            ix.search_filtered(q, 8193, THR, vhead, None)
        with pytest.raises(HipLibraryError, match="128 inputs, d_user is 256"):
            ix.search_filtered(q, 40, THR, narrow, None)
        with pytest.raises(HipLibraryError, match="128 inputs, d_user is 256"):
            ix.search_filtered(q, 40, THR, None, narrow)
        with pytest.raises(HipLibraryError, match="bias-free"):
            ix.search_filtered(q, 40, THR, biased, None)
        with pytest.raises(HipLibraryError, match="no filter asked for"):
            ix.search_filtered(q, 40, None, None, None)
        if torch.cuda.device_count() > 1:
            far = Mi355xSafetyHead({"layers.0.weight": prompts}, device=1, relu=[False])
            try:
                with pytest.raises(HipLibraryError, match="lives on device 1, the index on device 0"):
                    ix.search_filtered(q, 40, THR, far, None)
            finally:
                far.close()
        after = ix.search_filtered(q, 40, THR, vhead, None)
        for a, b in zip(before[:3], after[:3]):
            assert np.array_equal(a, b)
        assert before[3] == after[3]
    finally:
        for h in (vhead, narrow, biased):
            h.close()


def test_eight_filtered_callers_beside_eight_plain_searchers():
    from clip_retrieval_amd.knn import Mi355xIndex
    from clip_retrieval_amd.service import Mi355xSafetyHead

    d = 256
    x, _ = _corpus(d)
    rng = np.random.default_rng(81)
    ix = Mi355xIndex(d)  # (coalescing on: the plain searchers share scans while the filtered callers hold the index)
    ix.add(x)
    prompts, sd = _prompts(d, 82), _small_stack(d, 83)
    vhead, shead = Mi355xSafetyHead({"layers.0.weight": prompts}, relu=[False]), Mi355xSafetyHead(sd)
    qs = (x[rng.integers(0, 6000, 8)].astype(np.float32) + 0.05 * rng.standard_normal((8, d)).astype(np.float32))
    ks = [3000, 100, 40, 500, 3000, 65, 1000, 129]
    try:
        alone = [ix.search_filtered(qs[t][None], ks[t], THR, vhead, shead, 0.0) for t in range(8)]
        plain = [ix.search(qs[t][None], 40) for t in range(8)]
        assert any(np.any(a[2] & 1) for a in alone) and any(np.any(a[2] & 2) for a in alone) and any(np.any(a[2] & 4) for a in alone)
        errors = []

        def filtered(t):
            try:
                for _ in range(3):
                    got = ix.search_filtered(qs[t][None], ks[t], THR, vhead, shead, 0.0)
                    assert all(np.array_equal(a, b) for a, b in zip(got[:3], alone[t][:3])) and got[3] == alone[t][3]
            except BaseException as e:  # pylint: disable=broad-except
                errors.append(e)

        def searcher(t):
            try:
                for _ in range(12):
                    got = ix.search(qs[t][None], 40)
                    assert np.array_equal(got[0], plain[t][0]) and np.array_equal(got[1], plain[t][1])
            except BaseException as e:  # pylint: disable=broad-except
                errors.append(e)

        threads = [threading.Thread(target=f, args=(t,)) for t in range(8) for f in (filtered, searcher)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors[:3]
    finally:
        vhead.close(), shead.close()
        ix.close()
