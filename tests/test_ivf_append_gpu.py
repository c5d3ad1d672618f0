"""Growing a built IVF index (Mi355xIndex.ivf_append / ivf_append_device / merge_from, knn.append_new_folder_rows; include/knnx.h,
"Growing a built index") against the index the existing builders give from scratch over the concatenated rows with the same centroids,
quantiser and lists.  No tolerance anywhere: D, I, R, exported codes, id maps and reconstructed rows are compared bit for bit."""
import os
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from test_ivfsq_cpu import corpus, np_sq_encode
from test_ivfsq_gpu import N, NLIST, SIZES, _crafted, _queries

pytestmark = pytest.mark.gpu

# rows the first append gives every list: 0 -> 1 (the first list grows), 1 -> 32 (fills its tile exactly), 31 -> 32, 32 -> 33 (gains a
# tile), 33 -> 64, 700 -> 1000, 5 -> 32, 250 -> 256; the last list grows; list 9 is empty and stays empty; the others gain nothing
EXTRA = np.zeros(NLIST, dtype=np.int64)
for _l, _n in ((0, 1), (1, 31), (2, 1), (3, 1), (4, 31), (5, 300), (10, 27), (13, 6), (23, 7)):
    EXTRA[_l] = _n
NA = int(EXTRA.sum())
assert [int(SIZES[l]) for l in (0, 1, 2, 3, 4, 5, 9)] == [0, 1, 31, 32, 33, 700, 0] and EXTRA[9] == 0 and (EXTRA == 0).sum() >= 10
N2, N3 = 1, 97  # the second and third append

# kind, d, and what the variant switches on
VARIANTS = {
    "flat": dict(kind="flat", d=256),
    "pq": dict(kind="pq", d=256, M=16),
    "sq": dict(kind="sq", d=256),
    "pq-refine": dict(kind="pq", d=256, M=16, refine=True),
    "pq-rotation": dict(kind="pq", d=256, M=16, dq=256),
    "pq-rect-rotation": dict(kind="pq", d=256, M=16, dq=512),
    "pq-m256": dict(kind="pq", d=512, M=256),
    "pq-threshold": dict(kind="pq", d=256, M=16, thr=True),
    "sq-threshold": dict(kind="sq", d=256, thr=True),
    "sq-768": dict(kind="sq", d=768),     # a tile of 1536 uint4: one whole burst of the move kernel and a ragged rest
    "flat-512": dict(kind="flat", d=512),  # a tile of 2048 uint4: two whole bursts
}
_PARTS = {}


def _parts(d):
    """The crafted base of test_ivfsq_gpu.py (x, lists, cent, ranges) plus NA + N2 + N3 further rows of the same corpus and their lists:
    the first NA in shuffled order with EXTRA rows per list, then one row for list 3, then 97 rows over random lists."""
    if d not in _PARTS:
        x, lists, cent, ranges = _crafted(d)
        rng = np.random.default_rng(1000 + d)
        xa = corpus("mixture" if d == 256 else "isotropic", d, N + NA + N2 + N3)[N:].copy()
        la = np.repeat(np.arange(NLIST, dtype=np.int32), EXTRA)
        rng.shuffle(la)
        la = np.concatenate([la, np.asarray([3], np.int32), rng.integers(0, NLIST, N3).astype(np.int32)])
        _PARTS[d] = SimpleNamespace(x=x, lists=lists, cent=cent, ranges=ranges, xa=xa, la=la, q=_queries(200, d, 5, x))
    return _PARTS[d]


def _quantiser(v):
    """(centroids in the quantiser space, codebooks, rotation) of a PQ variant: random codebooks, a random orthonormal rotation."""
    p = _parts(v["d"])
    d, dq = v["d"], v.get("dq") or v["d"]
    rng = np.random.default_rng(v["M"] + dq)
    rot, cent = None, p.cent
    if "dq" in v:
        Q, _ = np.linalg.qr(rng.standard_normal((dq, d)))
        rot = np.ascontiguousarray(Q.astype(np.float32))
        c = p.cent.astype(np.float32) @ rot.T
        cent = (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float16)
    cb = (0.05 * rng.standard_normal((v["M"], 256, dq // v["M"]))).astype(np.float32)
    return cent, cb, rot


def _build(v, x, lists, id_base=0, cent=None, cb=None, ranges=None, refine=None):
    """The variant's index over these rows and lists, from scratch, by the builders every other test file pins to numpy."""
    from clip_retrieval_amd import knn

    p, d, n = _parts(v["d"]), v["d"], len(x)
    lists = np.ascontiguousarray(lists, dtype=np.int32)

    def chunks():
        return ((o, x[o:o + 1000]) for o in range(0, n, 1000))

    if v["kind"] == "flat":
        c = p.cent if cent is None else cent
        ix = knn._ivf_begin(knn.Mi355xIndex(d, id_base=id_base), NLIST, c, knn._list_sizes(lists, NLIST))  # pylint: disable=protected-access
        knn._add_assigned_chunks(ix, chunks(), lists, NLIST, id_base)  # pylint: disable=protected-access
        return knn._ivf_end(ix, NLIST, 5, c, id_base, n, lists)  # pylint: disable=protected-access
    if v["kind"] == "sq":
        return knn._ivfsq_encode_chunks(chunks(), n, d, NLIST, p.cent if cent is None else cent, p.ranges if ranges is None else ranges,  # pylint: disable=protected-access
                                        lists, 5, 0, id_base, v.get("thr", False))
    qc, qcb, rot = _quantiser(v)
    return knn._ivfpq_encode_chunks(chunks(), n, d, NLIST, v["M"], qc if cent is None else cent, qcb if cb is None else cb, lists, 5, 0,  # pylint: disable=protected-access
                                    id_base, rot, v.get("refine", False) if refine is None else refine, 4 if v.get("refine") else 1,
                                    v.get("thr", False))


def _threshold(ix, q):
    """A range_search threshold that a few dozen rows per query pass."""
    ix.nprobe = NLIST
    D, _ = ix.search(q[:5], 64)
    return float(np.median(D[:, 40]))


def _observe(ix, v, q, thresh=None, nprobes=(NLIST, 1, 5, NLIST)):
    """Everything the index answers, as a list of (name, array): B = 1, 32 and 200 searches (single-block, one block, multi-block),
    search_and_reconstruct, with the threshold scan on also k = 100 and a range_search -- at every nprobe --, the exported codes, both
    id maps, every row reconstructed, ntotal.  The default walk over nprobe ends where it starts, so the first search after an append
    runs at the nprobe of the last search before it: what is cached per nprobe (the M = 256 slab width) must not survive the append."""
    out = [("ntotal", np.asarray([ix.ntotal]))]
    for nprobe in nprobes:
        ix.nprobe = nprobe
        for B in (1, 32, 200):
            D, I = ix.search(q[:B], 10)
            out += [(f"D np{nprobe} B{B}", D), (f"I np{nprobe} B{B}", I)]
        D, I, R = ix.search_and_reconstruct(q[:32], 10)
        out += [(f"sar D np{nprobe}", D), (f"sar I np{nprobe}", I), (f"sar R np{nprobe}", R)]
        if v.get("thr"):
            D, I = ix.search(q[:5], 100)
            lims, Dr, Ir = ix.range_search(q[:5], thresh)
            assert lims[-1] > 0
            out += [(f"k100 D np{nprobe}", D), (f"k100 I np{nprobe}", I), (f"range lims np{nprobe}", lims), (f"range D np{nprobe}", Dr),
                    (f"range I np{nprobe}", Ir)]
    if v["kind"] != "flat":
        codes, lists = ix.pq_codes() if v["kind"] == "pq" else ix.sq_codes()
        out += [("codes", codes), ("code lists", lists)]
    lo = ix.ivf_row_range[0]
    out += [("new_to_old", ix.ivf_new_to_old()), ("old_to_new", ix.ivf_old_to_new()),
            ("reconstruct", ix.reconstruct_batch(np.arange(lo, lo + ix.ntotal, dtype=np.int64)))]
    return out


def _assert_same(got, want, ctx):
    assert [n for n, _ in got] == [n for n, _ in want], ctx
    for (name, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{ctx}: {name}: {a.dtype} {a.shape} against {b.dtype} {b.shape}"
        assert a.tobytes() == b.tobytes(), f"{ctx}: {name} differs in {int((np.asarray(a) != np.asarray(b)).sum())} entries"


# ------------------------------------------------------------------------------------------------ append with given lists
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_append_equals_a_fresh_build(name):
    """Caches warmed by every kind of call, then three appends (the crafted batch, 1 row, 97 rows): after the first and after the third
    the index answers everything exactly as the index built from scratch over the concatenated rows does."""
    v = VARIANTS[name]
    p = _parts(v["d"])
    ix = _build(v, p.x, p.lists)
    thresh = _threshold(ix, p.q) if v.get("thr") else None
    base = _observe(ix, v, p.q, thresh)  # warms ivf1 / ivfm / pqs / sqs / the threshold scratch / the hit pools / the list-order cache
    ids = ix.ivf_append(p.xa[:NA], lists=p.la[:NA])
    assert np.array_equal(ids, np.arange(N, N + NA)) and ids.dtype == np.int64 and ix.ntotal == N + NA
    x1, l1 = np.concatenate([p.x, p.xa[:NA]]), np.concatenate([p.lists, p.la[:NA]])
    assert np.array_equal(np.bincount(l1, minlength=NLIST), SIZES + EXTRA)
    fresh = _build(v, x1, l1)
    _assert_same(_observe(ix, v, p.q, thresh), _observe(fresh, v, p.q, thresh), f"{name}: first append")
    assert np.array_equal(ix.ivf_lists, l1) and ix.ivf_row_range == (0, N + NA)
    if v["kind"] == "sq":  # the appended rows' codes are numpy's
        assert np.array_equal(ix.sq_codes()[0][N:], np_sq_encode(p.xa[:NA], *p.ranges))
    if v["kind"] == "flat" or v.get("refine"):  # ... and stored rows come back exactly
        assert np.array_equal(ix.reconstruct_batch(ids), p.xa[:NA].astype(np.float32))
        assert np.array_equal(ix.reconstruct(N + 3), p.xa[3].astype(np.float32))
    fresh.close()
    ids2 = ix.ivf_append(p.xa[NA:NA + N2], lists=p.la[NA:NA + N2])
    ids3 = ix.ivf_append(p.xa[NA + N2:].astype(np.float32), lists=p.la[NA + N2:])  # (float32 rows are rounded to fp16 like add's)
    assert ids2.tolist() == [N + NA] and np.array_equal(ids3, np.arange(N + NA + N2, N + NA + N2 + N3))
    fresh = _build(v, np.concatenate([p.x, p.xa]), np.concatenate([p.lists, p.la]))
    _assert_same(_observe(ix, v, p.q, thresh), _observe(fresh, v, p.q, thresh), f"{name}: third append")
    # the base index's answers were not those of the grown one: the comparison above is not vacuous
    assert any(a.tobytes() != b.tobytes() for (_, a), (_, b) in zip(base[1:20], _observe(fresh, v, p.q, thresh)[1:20]))
    fresh.close()
    ix.close()


# ------------------------------------------------------------------------------------------------ the library assigns
@pytest.mark.parametrize("name", ["flat", "sq", "pq-rotation", "pq-rect-rotation"])
def test_library_assignment_and_device_rows(name):
    """ivf_append(x) without lists = IvfBuilder.assign of the rows (rotated first where the index has a rotation) followed by the
    crafted path; ivf_append_device of the same rows in HBM gives the same index."""
    import torch

    from clip_retrieval_amd.knn import IvfBuilder, rotate_rows

    v = VARIANTS[name]
    p = _parts(v["d"])
    xa = p.xa[:500]
    cent, rot = (p.cent, None) if v["kind"] != "pq" else (_quantiser(v)[0], _quantiser(v)[2])
    b = IvfBuilder(cent.shape[1], NLIST)
    b.set_centroids(cent)
    want = b.assign(xa if rot is None else rotate_rows(rot, xa))
    b.close()
    assert len(np.unique(want)) > 3
    fresh = _build(v, np.concatenate([p.x, xa]), np.concatenate([p.lists, want]))
    expect = _observe(fresh, v, p.q, nprobes=(5,))
    fresh.close()
    host = _build(v, p.x, p.lists)
    _observe(host, v, p.q, nprobes=(5,))
    assert np.array_equal(host.ivf_append(xa), np.arange(N, N + 500))
    assert np.array_equal(host.ivf_lists[N:], want)
    _assert_same(_observe(host, v, p.q, nprobes=(5,)), expect, f"{name}: library assignment")
    host.close()
    dev = _build(v, p.x, p.lists)
    xd = torch.from_numpy(xa).cuda()
    torch.cuda.synchronize()
    assert np.array_equal(dev.ivf_append_device(xd.data_ptr(), 500), np.arange(N, N + 500))
    assert np.array_equal(dev.ivf_lists[N:], want)
    _assert_same(_observe(dev, v, p.q, nprobes=(5,)), expect, f"{name}: device rows")
    dev.close()


def test_device_append_across_the_internal_chunk():
    """(1 << 20) + 33 rows made on the device go into an IVF-SQ8 index through ivf_append_device: the library walks them in chunks of
    2^20 rows and positions carry across the boundary.  Equal to build_ivfsq_index_device over all rows."""
    import torch

    from clip_retrieval_amd.knn import build_ivfsq_index_device, synth_rows_device

    d, n0, n1 = 256, 3000, (1 << 20) + 33
    p = _parts(d)

    def fill_rows(dst, row0, count, stride):
        synth_rows_device(dst, row0, count, d, 11, row_stride=stride)
        torch.cuda.synchronize()

    ix, _ = build_ivfsq_index_device(fill_rows, n0, d, NLIST, nprobe=5, centroids=p.cent, ranges=p.ranges, keep_lists=True)
    ix.search(p.q[:40], 10)
    rows = torch.empty((n1, d), dtype=torch.float16, device="cuda")
    fill_rows(rows.data_ptr(), n0, n1, 1)
    ids = ix.ivf_append_device(rows.data_ptr(), n1)
    assert ids[0] == n0 and ids[-1] == n0 + n1 - 1 and ix.ntotal == n0 + n1
    del rows
    fresh, _ = build_ivfsq_index_device(fill_rows, n0 + n1, d, NLIST, nprobe=5, centroids=p.cent, ranges=p.ranges, keep_lists=True)
    assert np.array_equal(ix.ivf_lists, fresh.ivf_lists)
    assert np.array_equal(ix.ivf_new_to_old(), fresh.ivf_new_to_old())
    for a, b in zip(ix.sq_codes(), fresh.sq_codes()):
        assert np.array_equal(a, b)
    for B in (1, 200):
        (D0, I0), (D1, I1) = ix.search(p.q[:B], 10), fresh.search(p.q[:B], 10)
        assert np.array_equal(I0, I1) and D0.tobytes() == D1.tobytes()
    ix.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------ merge_from
H = 1301  # the crafted rows split here, in the middle of most lists


@pytest.mark.parametrize("name,base_a,base_b", [("flat", 0, 0), ("pq", 0, 0), ("sq", 0, 0), ("pq-refine", 0, 0), ("sq", 1000, 77),
                                                ("flat", 1000, 77)])
def test_merge_from_equals_a_fresh_build(name, base_a, base_b):
    """The crafted rows in two indexes with shared quantisers, the second merged into the first = the build over all rows; the
    second index (with an id_base of its own in two cases) is left as it was."""
    v = VARIANTS[name]
    p = _parts(v["d"])
    a = _build(v, p.x[:H], p.lists[:H], id_base=base_a)
    b = _build(v, p.x[H:], p.lists[H:], id_base=base_b)
    _observe(a, v, p.q)
    before_b = _observe(b, v, p.q, nprobes=(5,))
    ids = a.merge_from(b)
    assert np.array_equal(ids, np.arange(base_a + H, base_a + N)) and a.ntotal == N
    fresh = _build(v, p.x, p.lists, id_base=base_a)
    _assert_same(_observe(a, v, p.q), _observe(fresh, v, p.q), f"{name}: merged")
    assert np.array_equal(a.ivf_lists, p.lists) and a.ivf_row_range == (base_a, base_a + N)
    _assert_same(_observe(b, v, p.q, nprobes=(5,)), before_b, f"{name}: the merged-from index changed")
    for ix in (a, b, fresh):
        ix.close()


def test_merge_refusals_leave_the_index_as_it_was():
    from clip_retrieval_amd import HipLibraryError

    p = _parts(256)
    sq, pq, flat = VARIANTS["sq"], VARIANTS["pq"], VARIANTS["flat"]
    cent2 = p.cent.copy()
    cent2[3, 5] = np.float16(float(cent2[3, 5]) + 0.25)
    ranges2 = (p.ranges[0], p.ranges[1] * np.float32(1.5))
    qc, qcb, _ = _quantiser(pq)
    cb2 = qcb.copy()
    cb2[2, 9, 1] += 1.0
    part = (p.x[H:], p.lists[H:])
    a_sq, a_pq, a_flat = _build(sq, p.x[:H], p.lists[:H]), _build(pq, p.x[:H], p.lists[:H]), _build(flat, p.x[:H], p.lists[:H])
    cases = [
        (a_sq, sq, _build(sq, *part, cent=cent2), "centroids"),
        (a_sq, sq, _build(sq, *part, ranges=ranges2), "ranges"),
        (a_pq, pq, _build(pq, *part, cb=cb2), "codebooks"),
        (a_pq, pq, _build(pq, *part, cent=cent2), "centroids"),
        (a_pq, pq, _build(pq, *part, refine=True), "refine"),
        (a_pq, pq, _build(sq, *part), "kind"),
        (a_flat, flat, _build(sq, *part), "kind"),
        (a_flat, flat, _build(flat, *part, cent=cent2), "centroids"),
        (a_sq, sq, a_sq, "itself"),
    ]
    before = {id(ix): _observe(ix, v, p.q, nprobes=(5,)) for ix, v in ((a_sq, sq), (a_pq, pq), (a_flat, flat))}
    for ix, v, other, word in cases:
        with pytest.raises(HipLibraryError, match=word) as e:
            ix.merge_from(other)
        assert "code -1" in str(e.value) and "nothing was added" in str(e.value), str(e.value)
        _assert_same(_observe(ix, v, p.q, nprobes=(5,)), before[id(ix)], f"refused merge ({word})")
        if other is not ix:
            other.close()
    with pytest.raises(TypeError):
        a_sq.merge_from(object())
    for ix in (a_sq, a_pq, a_flat):
        ix.close()


# ------------------------------------------------------------------------------------------------ refusals of append
@pytest.mark.parametrize("name", ["flat", "pq", "sq"])
def test_append_refusals_change_nothing(name):
    from clip_retrieval_amd import HipLibraryError, knn

    v = VARIANTS[name]
    p = _parts(v["d"])
    ix = _build(v, p.x, p.lists)
    before = _observe(ix, v, p.q, nprobes=(5,))
    bad = p.la[:50].copy()
    bad[49] = NLIST
    with pytest.raises(HipLibraryError, match="list id out of range"):
        ix.ivf_append(p.xa[:50], lists=bad)
    bad[49] = -1
    with pytest.raises(HipLibraryError, match="nothing was added"):
        ix.ivf_append(p.xa[:50], lists=bad)
    with pytest.raises(ValueError):
        ix.ivf_append(np.zeros((4, v["d"] + 1), np.float16))
    with pytest.raises(ValueError):
        ix.ivf_append(p.xa[:50], lists=p.la[:49])
    with pytest.raises(TypeError):
        ix.ivf_append(np.zeros((4, v["d"]), np.int32))
    assert ix.ivf_append(np.zeros((0, v["d"]), np.float16)).shape == (0,)
    _assert_same(_observe(ix, v, p.q, nprobes=(5,)), before, f"{name}: refused appends")
    assert ix.ntotal == N and len(ix.ivf_lists) == N and ix.ivf_row_range == (0, N)
    # add() on a built IVF index still raises what it raised
    word = "rebuild the index instead" if name == "flat" else "rows are encoded by knnx_ivf_begin"
    with pytest.raises(HipLibraryError, match=word):
        ix.add(p.xa[:4])
    _assert_same(_observe(ix, v, p.q, nprobes=(5,)), before, f"{name}: refused add")
    ix.close()
    # a flat index, and an index between knnx_ivf_begin and knnx_ivf_end
    plain = knn.Mi355xIndex(v["d"])
    plain.add(p.x[:100])
    D0, I0 = plain.search(p.q[:5], 10)
    for call in (lambda: plain.ivf_append(p.xa[:5]), lambda: plain.ivf_append(p.xa[:5], lists=p.la[:5])):
        with pytest.raises(HipLibraryError, match="not a built IVF index"):
            call()
    D1, I1 = plain.search(p.q[:5], 10)
    assert plain.ntotal == 100 and np.array_equal(I0, I1) and D0.tobytes() == D1.tobytes()
    plain.close()
    if name == "flat":
        opened = knn._ivf_begin(knn.Mi355xIndex(v["d"]), NLIST, p.cent, SIZES)  # pylint: disable=protected-access
        with pytest.raises(HipLibraryError, match="between knnx_ivf_begin and knnx_ivf_end"):
            opened.ivf_append(p.xa[:5], lists=p.la[:5])
        knn._add_assigned_chunks(opened, [(0, p.x)], p.lists, NLIST, 0)  # pylint: disable=protected-access
        knn._ivf_end(opened, NLIST, 5, p.cent, 0, N, p.lists)  # pylint: disable=protected-access
        _assert_same(_observe(opened, v, p.q, nprobes=(5,)), before, "the build the refused append interrupted")
        opened.close()


# ------------------------------------------------------------------------------------------------ searches while the index grows
@pytest.mark.parametrize("name", ["sq", "flat"])
def test_searches_during_appends_see_one_of_the_states(name):
    """Four threads search (B = 1) in a loop while the main thread appends three times: no call raises, and every answer is the
    answer of one of the four states of the index, each computed from a fresh build."""
    v = VARIANTS[name]
    p = _parts(v["d"])
    cuts = [0, NA, NA + N2, NA + N2 + N3]
    # thread t asks for the neighbours of the sum of a row of the first batch and a row of the third: its answer changes when either arrives
    q = p.xa[[0, 1, 2, 3]].astype(np.float32) + p.xa[[NA + N2 + 5 * t for t in range(4)]].astype(np.float32)
    q = np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True))
    want = []
    for c in cuts:  # the four states, from scratch
        s = _build(v, np.concatenate([p.x, p.xa[:c]]), np.concatenate([p.lists, p.la[:c]]))
        s.nprobe = NLIST
        want.append([s.search(q[t:t + 1], 10) for t in range(4)])
        s.close()
    for t in range(4):  # (the one row of the second append need not show)
        assert (N + t) in want[1][t][1] and (N + t) not in want[0][t][1], "the first batch must show"
        assert not np.array_equal(want[2][t][1], want[3][t][1]), "the third batch must show"
    ix = _build(v, p.x, p.lists)
    ix.nprobe = NLIST
    stop, started = threading.Event(), threading.Barrier(5)
    got, errors = [[] for _ in range(4)], []

    def worker(t):
        try:
            started.wait()
            while True:
                last = stop.is_set()
                got[t].append(ix.search(q[t:t + 1], 10))
                if last:
                    return
        except Exception as e:  # pylint: disable=broad-except
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    started.wait()
    for a, b in zip(cuts[:-1], cuts[1:]):
        ix.ivf_append(p.xa[a:b], lists=p.la[a:b])
    stop.set()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(4):
        states = [next((s for s in range(4) if D.tobytes() == want[s][t][0].tobytes() and I.tobytes() == want[s][t][1].tobytes()), None)
                  for D, I in got[t]]
        assert None not in states, f"thread {t}: answer {states.index(None)} of {len(states)} belongs to no state of the index"
        assert states == sorted(states), f"thread {t}: {states}"
        D, I = got[t][-1]  # (started after the last append returned)
        assert D.tobytes() == want[3][t][0].tobytes() and I.tobytes() == want[3][t][1].tobytes(), f"thread {t}: the last search missed the last append"
    ix.close()


# ------------------------------------------------------------------------------------------------ folders
def _write_files(folder, parts):
    os.makedirs(folder, exist_ok=True)
    for i, a in parts:
        np.save(os.path.join(folder, f"img_emb_{i:04d}.npy"), a)


@pytest.mark.parametrize("name", ["flat", "pq-refine", "sq"])
def test_folder_round_trip(tmp_path, name):
    """Build from a two-file folder, save, a third file arrives, append_new_folder_rows, save, load_index = the build over the three
    files with the same centroids and quantiser."""
    from clip_retrieval_amd import knn

    v = VARIANTS[name]
    p = _parts(v["d"])
    emb, s1, s2 = str(tmp_path / "emb"), str(tmp_path / "saved1"), str(tmp_path / "saved2")
    third = p.xa[:NA]

    def build(folder):
        if v["kind"] == "flat":
            return knn.build_ivf_index_from_folder(folder, NLIST, nprobe=5, centroids=p.cent)
        if v["kind"] == "sq":
            return knn.build_ivfsq_index_from_folder(folder, NLIST, nprobe=5, centroids=p.cent, ranges=p.ranges)
        qc, qcb, _ = _quantiser(v)
        return knn.build_ivfpq_index_from_folder(folder, NLIST, v["M"], nprobe=5, centroids=qc, codebooks=qcb, refine=True, k_factor=4)

    _write_files(emb, [(0, p.x[:1500]), (1, p.x[1500:])])
    ix = build(emb)
    knn.save_index(ix, s1, embeddings_folder=emb)
    assert knn.append_new_folder_rows(ix).shape == (0,)  # nothing new yet
    _write_files(emb, [(2, third)])
    ids = knn.append_new_folder_rows(ix)
    assert np.array_equal(ids, np.arange(N, N + NA)) and ix.ntotal == N + NA
    knn.save_index(ix, s2, embeddings_folder=emb)
    loaded = knn.load_index(s2)  # (the flat and the refine folder find the embeddings at the path they recorded)
    fresh = build(emb)
    want = _observe(fresh, v, p.q, nprobes=(5,))
    _assert_same(_observe(ix, v, p.q, nprobes=(5,)), want, f"{name}: appended from the folder")
    _assert_same(_observe(loaded, v, p.q, nprobes=(5,)), want, f"{name}: saved and loaded")
    assert np.array_equal(np.asarray(loaded.ivf_lists), np.asarray(fresh.ivf_lists))
    # a changed old file is refused, and nothing is added
    _write_files(emb, [(1, p.x[1500:-1]), (3, third[:5])])
    with pytest.raises(ValueError, match="changed"):
        knn.append_new_folder_rows(ix)
    assert ix.ntotal == N + NA
    for i in (ix, loaded, fresh):
        i.close()
