"""Shrinking a built IVF index (Mi355xIndex.ivf_remove / remove_ids; include/knnx.h, "Shrinking a built index") against the index the
existing builders give from scratch over the surviving rows, in their original order, with the same centroids, quantiser and lists.
No tolerance anywhere: D, I, R, exported codes, id maps and reconstructed rows are compared bit for bit."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from test_ivf_append_gpu import VARIANTS, _assert_same, _build, _observe, _parts, _threshold
from test_ivf_append_gpu import NA, N2
from test_ivfsq_gpu import N, NLIST, SIZES

pytestmark = pytest.mark.gpu

assert SIZES.tolist() == [0, 1, 31, 32, 33, 700, 64, 65, 96, 0, 5, 130, 17, 250, 2, 63, 40, 128, 90, 11, 160, 75, 1, 300] and N == 2294
FLT_MIN = np.finfo(np.float32).min  # the score padding of a short result (-FLT_MAX)


def _at(lists, l, positions):
    """The ids at these positions of list l: position j is the j-th smallest id of the list."""
    return np.flatnonzero(np.asarray(lists) == l)[np.asarray(positions, dtype=np.int64)]


def _crafted_set(lists):
    """List 1 loses its only row (and its only tile); list 2 position 0 (30 rows shift inside one tile); list 3 position 31 (32 -> 31);
    list 4 position 0 (33 -> 32: the row of the second tile crosses into the first, the list loses a tile); list 5 its whole second
    tile, positions 0 and 699 and every third from 100 to 400; list 6 every even position (64 -> 32, loses a tile); list 7 all 65
    rows (an empty list in the middle of the arena); list 8 its whole first tile; list 13 all but position 249 (250 -> 1); list 23
    position 299, the last occupied row of the arena.  Lists 0 and 9 are empty; 10, 11, 12 and 14 .. 22 lose nothing."""
    parts = [_at(lists, 1, [0]), _at(lists, 2, [0]), _at(lists, 3, [31]), _at(lists, 4, [0]),
             _at(lists, 5, list(range(32, 64)) + [0, 699] + list(range(100, 401, 3))), _at(lists, 6, range(0, 64, 2)),
             _at(lists, 7, range(65)), _at(lists, 8, range(32)), _at(lists, 13, range(249)), _at(lists, 23, [299])]
    s = np.concatenate(parts).astype(np.int64)
    assert len(np.unique(s)) == len(s)
    return s


def _grow_stats(ix):
    v = [C.c_double() for _ in range(4)] + [C.c_int64()]
    assert ix._lib.knnx_ivf_grow_stats(ix._h, *[C.byref(a) for a in v]) == 0  # pylint: disable=protected-access
    return [a.value for a in v]


# ------------------------------------------------------------------------------------------------ removal = a fresh build
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_remove_equals_a_fresh_build(name):
    """Caches warmed by every kind of call, then three removals (the crafted set, the row with new id 0, 97 random ids with duplicates
    and ids that name no row): after the first and after the third the index answers everything exactly as the index built from
    scratch over the surviving rows does."""
    v = VARIANTS[name]
    p = _parts(v["d"])
    ix = _build(v, p.x, p.lists)
    thresh = _threshold(ix, p.q) if v.get("thr") else None
    base = _observe(ix, v, p.q, thresh)  # warms ivf1 / ivfm / pqs / sqs / the threshold scratch / the hit pools / the list-order cache
    S = _crafted_set(p.lists)
    rng = np.random.default_rng(7)
    kept = ix.ivf_remove(rng.permutation(S).reshape(2, -1) if len(S) % 2 == 0 else rng.permutation(S))
    assert kept.dtype == np.int64 and np.array_equal(kept, np.setdiff1d(np.arange(N), S)) and ix.ntotal == N - len(S)
    sizes1 = np.bincount(p.lists[kept], minlength=NLIST)
    assert sizes1[[1, 2, 3, 4, 6, 7, 8, 13, 23]].tolist() == [0, 30, 31, 32, 32, 0, 64, 1, 299] and sizes1[0] == sizes1[9] == 0
    assert ((sizes1 == SIZES) & (SIZES > 0)).sum() >= 10, "at least 10 lists must be untouched"
    fresh = _build(v, p.x[kept], p.lists[kept])
    _assert_same(_observe(ix, v, p.q, thresh), _observe(fresh, v, p.q, thresh), f"{name}: first removal")
    assert np.array_equal(ix.ivf_lists, p.lists[kept]) and ix.ivf_row_range == (0, N - len(S))
    if v["kind"] == "flat" or v.get("refine"):  # stored rows come back exactly, under their new ids
        assert np.array_equal(ix.reconstruct_batch(np.arange(len(kept), dtype=np.int64)), p.x[kept].astype(np.float32))
    fresh.close()
    rows = kept.copy()  # the original row number of every row the index holds, in id order
    kept2 = ix.ivf_remove([0])
    assert np.array_equal(kept2, np.arange(1, len(rows)))
    rows = rows[kept2]
    id_base = 0
    ids3 = np.concatenate([rng.integers(0, len(rows), 97), [-1, id_base - 1, ix.ntotal + 5]]).astype(np.int64)
    gone = np.unique(ids3[(ids3 >= 0) & (ids3 < len(rows))])
    assert len(gone) < 97, "the random ids must hold duplicates"
    assert ix.remove_ids(ids3) == len(gone)
    rows = np.delete(rows, gone)
    assert ix.ntotal == len(rows)
    fresh = _build(v, p.x[rows], p.lists[rows])
    final = _observe(fresh, v, p.q, thresh)
    _assert_same(_observe(ix, v, p.q, thresh), final, f"{name}: third removal")
    assert np.array_equal(ix.ivf_lists, p.lists[rows]) and ix.ivf_row_range == (0, len(rows))
    # the base index's answers were not those of the shrunken one: the comparison above is not vacuous
    assert any(a.tobytes() != b.tobytes() for (_, a), (_, b) in zip(base[1:20], final[1:20]))
    fresh.close()
    ix.close()


@pytest.mark.parametrize("name,id_base", [("sq", 1000), ("flat", 77)])
def test_remove_with_an_id_base(name, id_base):
    """New ids start at id_base, ids below it name no row, and reconstruct of a new id is the stored row."""
    v = VARIANTS[name]
    p = _parts(v["d"])
    ix = _build(v, p.x, p.lists, id_base=id_base)
    _observe(ix, v, p.q, nprobes=(5,))
    S = _crafted_set(p.lists)
    ids = np.concatenate([S + id_base, [id_base - 1, -1, id_base + N, 3]])  # (3 is below either id_base)
    kept = ix.ivf_remove(ids)
    assert np.array_equal(kept, id_base + np.setdiff1d(np.arange(N), S)) and ix.ivf_row_range == (id_base, id_base + len(kept))
    rows = kept - id_base
    fresh = _build(v, p.x[rows], p.lists[rows], id_base=id_base)
    _assert_same(_observe(ix, v, p.q, nprobes=(5, NLIST)), _observe(fresh, v, p.q, nprobes=(5, NLIST)), f"{name}: id_base {id_base}")
    assert np.array_equal(np.sort(ix.ivf_new_to_old()), np.arange(id_base, id_base + len(kept)))
    for i in (0, 1, len(kept) // 2, len(kept) - 1):
        if name == "flat":
            assert np.array_equal(ix.reconstruct(id_base + i), p.x[rows[i]].astype(np.float32))
        assert np.array_equal(ix.reconstruct(id_base + i), fresh.reconstruct(id_base + i))
    fresh.close()
    ix.close()


@pytest.mark.parametrize("name", ["flat", "pq-refine", "sq"])
def test_append_and_remove_interleave(name):
    v = VARIANTS[name]
    p = _parts(v["d"])
    ix = _build(v, p.x, p.lists)
    _observe(ix, v, p.q, nprobes=(5,))
    ix.ivf_append(p.xa[:NA], lists=p.la[:NA])
    X, L = np.concatenate([p.x, p.xa[:NA]]), np.concatenate([p.lists, p.la[:NA]])
    S = np.concatenate([_crafted_set(p.lists), N + np.asarray([0, 5, 6, 7, 100, NA - 1])])  # old and appended ids
    kept = ix.ivf_remove(S)
    assert np.array_equal(kept, np.setdiff1d(np.arange(N + NA), S))
    X, L = X[kept], L[kept]
    ids = ix.ivf_append(p.xa[NA + N2:], lists=p.la[NA + N2:])
    assert np.array_equal(ids, np.arange(len(kept), len(kept) + 97)), "the new ids start at the shrunken ntotal"
    X, L = np.concatenate([X, p.xa[NA + N2:]]), np.concatenate([L, p.la[NA + N2:]])
    fresh = _build(v, X, L)
    _assert_same(_observe(ix, v, p.q), _observe(fresh, v, p.q), f"{name}: append, remove, append")
    assert np.array_equal(ix.ivf_lists, L) and ix.ivf_row_range == (0, len(X))
    fresh.close()
    ix.close()


@pytest.mark.parametrize("name", ["flat", "pq"])
def test_remove_everything_then_append(name):
    v = VARIANTS[name]
    p = _parts(v["d"])
    ix = _build(v, p.x, p.lists)
    _observe(ix, v, p.q, nprobes=(5,))
    kept = ix.ivf_remove(np.arange(N))
    assert kept.shape == (0,) and ix.ntotal == 0 and len(ix.ivf_lists) == 0 and ix.ivf_row_range == (0, 0)
    for nprobe in (1, NLIST):
        ix.nprobe = nprobe
        for B in (1, 32, 200):
            D, I = ix.search(p.q[:B], 10)
            assert (I == -1).all() and (D == FLT_MIN).all()
    if name == "flat":
        lims, Dr, Ir = ix.range_search(p.q[:5], -1.0)
        assert lims.tolist() == [0] * 6 and len(Dr) == 0 and len(Ir) == 0
    assert ix.remove_ids(np.arange(10)) == 0  # nothing left to name
    ids = ix.ivf_append(p.xa[:200], lists=p.la[:200])
    assert np.array_equal(ids, np.arange(200))
    fresh = _build(v, p.xa[:200], p.la[:200])
    _assert_same(_observe(ix, v, p.q), _observe(fresh, v, p.q), f"{name}: emptied, then 200 rows")
    fresh.close()
    ix.close()


def test_nothing_to_remove_changes_nothing():
    from clip_retrieval_amd import HipLibraryError

    v = VARIANTS["sq"]
    p = _parts(v["d"])
    ix = _build(v, p.x, p.lists)
    before = _observe(ix, v, p.q, nprobes=(5,))
    with pytest.raises(HipLibraryError, match="nothing has been removed"):
        ix.ivf_remove_stats()
    assert ix.remove_ids(np.zeros(0, np.int64)) == 0
    assert ix.ivf_remove_stats()["moved_bytes"] == 0
    kept = ix.ivf_remove(np.asarray([[-1, N], [N + 5, -7]]))
    assert np.array_equal(kept, np.arange(N))
    st = ix.ivf_remove_stats()
    assert st["moved_bytes"] == 0 and st["n_removed"] == 0
    _assert_same(_observe(ix, v, p.q, nprobes=(5,)), before, "nothing to remove")
    assert ix.ntotal == N and np.array_equal(ix.ivf_lists, p.lists) and ix.ivf_row_range == (0, N)
    assert ix.remove_ids([5]) == 1  # and after a removal that moves rows the stats say so
    st = ix.ivf_remove_stats()
    assert st["n_removed"] == 1 and st["moved_bytes"] == (N - 1) * v["d"]
    ix.close()


def test_remove_refusals_change_nothing():
    from clip_retrieval_amd import HipLibraryError, knn

    v = VARIANTS["flat"]
    p = _parts(v["d"])
    # a flat index
    plain = knn.Mi355xIndex(v["d"])
    plain.add(p.x[:100])
    D0, I0 = plain.search(p.q[:5], 10)
    for ids in ([3], np.zeros(0, np.int64)):
        with pytest.raises(HipLibraryError, match="not a built IVF index") as e:
            plain.ivf_remove(ids)
        assert "code -1" in str(e.value) and "nothing was removed" in str(e.value)
    D1, I1 = plain.search(p.q[:5], 10)
    assert plain.ntotal == 100 and np.array_equal(I0, I1) and D0.tobytes() == D1.tobytes()
    plain.close()
    ix = _build(v, p.x, p.lists)
    before = _observe(ix, v, p.q, nprobes=(5,))
    # an index between knnx_ivf_begin and knnx_ivf_end
    opened = knn._ivf_begin(knn.Mi355xIndex(v["d"]), NLIST, p.cent, SIZES)  # pylint: disable=protected-access
    with pytest.raises(HipLibraryError, match="between knnx_ivf_begin and knnx_ivf_end") as e:
        opened.ivf_remove([0])
    assert "nothing was removed" in str(e.value)
    knn._add_assigned_chunks(opened, [(0, p.x)], p.lists, NLIST, 0)  # pylint: disable=protected-access
    knn._ivf_end(opened, NLIST, 5, p.cent, 0, N, p.lists)  # pylint: disable=protected-access
    _assert_same(_observe(opened, v, p.q, nprobes=(5,)), before, "the build the refused removal interrupted")
    opened.close()
    # a float array; NULL ids with n > 0 and a negative n through the raw entry point
    with pytest.raises(TypeError):
        ix.ivf_remove(np.asarray([1.0, 2.0]))
    lib, got = ix._lib, C.c_int64(-5)  # pylint: disable=protected-access
    for n in (3, -1):
        assert lib.knnx_ivf_remove_ids(ix._h, None, n, C.byref(got)) == -1  # pylint: disable=protected-access
        assert b"nothing was removed" in lib.knnx_last_error() and got.value == -5
    _assert_same(_observe(ix, v, p.q, nprobes=(5,)), before, "refused removals")
    assert ix.ntotal == N and len(ix.ivf_lists) == N and ix.ivf_row_range == (0, N)
    # add() and ivf_append behave as before
    with pytest.raises(HipLibraryError, match="rebuild the index instead"):
        ix.add(p.xa[:4])
    assert np.array_equal(ix.ivf_append(p.xa[:NA], lists=p.la[:NA]), np.arange(N, N + NA))
    fresh = _build(v, np.concatenate([p.x, p.xa[:NA]]), np.concatenate([p.lists, p.la[:NA]]))
    _assert_same(_observe(ix, v, p.q, nprobes=(5,)), _observe(fresh, v, p.q, nprobes=(5,)), "append after refused removals")
    fresh.close()
    ix.close()


# ------------------------------------------------------------------------------------------------ searches while the index shrinks
@pytest.mark.parametrize("name", ["sq", "flat"])
def test_searches_during_removals_see_one_of_the_states(name):
    """Four threads search (B = 1) in a loop while the main thread removes three times: no call raises, and every answer is the answer
    of one of the four states of the index, each computed from a fresh build."""
    v = VARIANTS[name]
    p = _parts(v["d"])
    a, b = _at(p.lists, 11, [0, 1, 2, 3]), _at(p.lists, 17, [0, 1, 2, 3])  # thread t asks for the neighbours of row a[t] + row b[t]
    q = p.x[a].astype(np.float32) + p.x[b].astype(np.float32)
    q = np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True))
    # the removals in original row numbers: the crafted set and the rows a; the first row left; the rows b and 20 rows of list 20
    states = [np.arange(N)]
    states.append(np.setdiff1d(states[0], np.concatenate([_crafted_set(p.lists), a])))
    states.append(states[1][1:])
    states.append(np.setdiff1d(states[2], np.concatenate([b, _at(p.lists, 20, range(20))])))
    calls = [np.searchsorted(s0, np.setdiff1d(s0, s1)) for s0, s1 in zip(states[:-1], states[1:])]  # the ids each call names
    want = []
    for rows in states:  # the four states, from scratch
        s = _build(v, p.x[rows], p.lists[rows])
        s.nprobe = NLIST
        want.append([s.search(q[t:t + 1], 10) for t in range(4)])
        s.close()
    for t in range(4):
        for s in range(3):
            assert want[s][t][1].tobytes() != want[s + 1][t][1].tobytes(), "every removal must show"
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
    for ids in calls:
        assert ix.remove_ids(ids) == len(ids)
    stop.set()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(4):
        seen = [next((s for s in range(4) if D.tobytes() == want[s][t][0].tobytes() and I.tobytes() == want[s][t][1].tobytes()), None)
                for D, I in got[t]]
        assert None not in seen, f"thread {t}: answer {seen.index(None)} of {len(seen)} belongs to no state of the index"
        assert seen == sorted(seen), f"thread {t}: {seen}"
        assert seen[-1] == 3, f"thread {t}: the last search missed the last removal"
    ix.close()


# ------------------------------------------------------------------------------------------------ folders
def _write_files(folder, parts):
    os.makedirs(folder, exist_ok=True)
    for i, a in parts:
        np.save(os.path.join(folder, f"img_emb_{i:04d}.npy"), a)


@pytest.mark.parametrize("name", ["pq", "sq", "flat", "pq-refine"])
def test_save_and_load_after_a_removal(tmp_path, name):
    """IVF-PQ without a refine store and IVF-SQ8 save as they always did; IVF-Flat and a refine index no longer belong to the folder
    they were built from and need embeddings_folder= naming a folder that holds the surviving rows.  The loaded index answers as the
    shrunken one.  knnx_ivf_grow_stats keeps its answer over a removal."""
    from clip_retrieval_amd import knn
    from test_ivf_append_gpu import _quantiser

    v = VARIANTS[name]
    p = _parts(v["d"])
    emb, emb2, saved = str(tmp_path / "emb"), str(tmp_path / "kept"), str(tmp_path / "saved")
    _write_files(emb, [(0, p.x[:1500]), (1, p.x[1500:])])
    if v["kind"] == "flat":
        ix = knn.build_ivf_index_from_folder(emb, NLIST, nprobe=5, centroids=p.cent)
    elif v["kind"] == "sq":
        ix = knn.build_ivfsq_index_from_folder(emb, NLIST, nprobe=5, centroids=p.cent, ranges=p.ranges)
    else:
        qc, qcb, _ = _quantiser(v)
        ix = knn.build_ivfpq_index_from_folder(emb, NLIST, v["M"], nprobe=5, centroids=qc, codebooks=qcb, refine=bool(v.get("refine")),
                                               k_factor=4 if v.get("refine") else 1)
    ix.ivf_append(p.xa[:5], lists=np.asarray(ix.ivf_lists[:5]))  # (so that the index has grow stats)
    grew = _grow_stats(ix)
    kept = ix.ivf_remove(np.concatenate([_crafted_set(p.lists), np.arange(N, N + 5)]))
    assert _grow_stats(ix) == grew
    assert np.array_equal(kept, np.setdiff1d(np.arange(N), _crafted_set(p.lists)))
    assert not any(hasattr(ix, a) for a in ("ivf_source", "embeddings_folder", "ivf_folder", "ivf_folder_files"))
    if name in ("flat", "pq-refine"):
        with pytest.raises(ValueError):
            knn.save_index(ix, saved)
        _write_files(emb2, [(0, p.x[kept][:1000]), (1, p.x[kept][1000:])])
        knn.save_index(ix, saved, embeddings_folder=emb2)
    else:
        knn.save_index(ix, saved)
    loaded = knn.load_index(saved)
    _assert_same(_observe(loaded, v, p.q, nprobes=(5,)), _observe(ix, v, p.q, nprobes=(5,)), f"{name}: saved and loaded after a removal")
    fresh = _build(v, p.x[kept], np.asarray(ix.ivf_lists))  # (the lists the folder builder assigned, filtered by the removal)
    _assert_same(_observe(ix, v, p.q, nprobes=(5,)), _observe(fresh, v, p.q, nprobes=(5,)), f"{name}: against the fresh build")
    for i in (ix, loaded, fresh):
        i.close()
