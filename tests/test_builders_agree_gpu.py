"""Three routes, one index: the same 5000 x 256 rows as a host array, as an embeddings folder of two partition files (3000 + 2000 rows)
and produced on the device through fill_rows must give, for every index kind, bit-equal codes and lists, bit-equal search results,
and -- for the two routes whose indexes can be saved -- byte-identical save_index folders."""
import json
import os

import numpy as np
import pytest

from build_cases import CHUNK, D, M, N, NLIST, corpus, fill_rows

pytestmark = pytest.mark.gpu

PATH_KEYS = ("embeddings_relative",)  # (and "folder" inside "embeddings"): where the embeddings are, not what the index is


def _build(kind, route, emb):
    from clip_retrieval_amd import knn

    c = corpus()
    kw = dict(nprobe=NLIST, chunk=CHUNK, centroids=c["cent"])
    if kind == "pq":
        kw["codebooks"] = c["codebooks"]
    elif kind == "sq":
        kw["ranges"] = c["ranges"]
    lead = (NLIST, M) if kind == "pq" else (NLIST,)
    name = {"flat": "build_ivf_index", "pq": "build_ivfpq_index", "sq": "build_ivfsq_index"}[kind]
    if route == "array":
        return getattr(knn, name)(c["x"], *lead, **kw)
    if route == "folder":
        return getattr(knn, name + "_from_folder")(emb, *lead, **kw)
    if kind == "flat":  # (the flat device builder takes no centroids: it is handed a sample that IS the centroids, see below)
        return _flat_device(c)
    if kind == "sq":
        kw["keep_lists"] = True
    return getattr(knn, name + "_device")(fill_rows, N, D, *lead, **kw)[0]


def _flat_device(c):
    """build_ivf_index_device always trains.  With niter = 0 its k-means only seeds, list l from sample row l when the sample has
    exactly nlist rows; a fill_rows that answers the strided sample request with the given centroids therefore builds with them."""
    import torch

    from clip_retrieval_amd import knn

    cent = torch.from_numpy(np.array(c["cent"])).cuda()

    def fill(dst, row0, count, stride):
        if stride > 1:
            assert count == NLIST
            _copy_to(dst, cent)
        else:
            fill_rows(dst, row0, count, stride)

    return knn.build_ivf_index_device(fill, N, D, NLIST, nprobe=NLIST, niter=0, chunk=CHUNK, sample_rows=NLIST, keep_lists=True)[0]


def _copy_to(dst_ptr, src):
    import ctypes as C

    import torch

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    torch.cuda.synchronize(0)
    assert hip.hipMemcpy(C.c_void_p(int(dst_ptr)), C.c_void_p(src.data_ptr()), src.numel() * src.element_size(), 3) == 0  # device to device
    torch.cuda.synchronize(0)  # (a device-to-device hipMemcpy does not wait on the host)


def _codes(kind, index):
    if kind == "pq":
        return index.pq_codes()
    if kind == "sq":
        return index.sq_codes()
    return (np.asarray(index.ivf_lists),)


def _manifest_without_paths(path):
    with open(path, encoding="utf-8") as f:
        man = json.load(f)
    for k in PATH_KEYS:
        man.pop(k, None)
    if isinstance(man.get("embeddings"), dict):
        man["embeddings"].pop("folder", None)
    return json.dumps(man, indent=1)  # (dicts keep the file's key order: the order is compared too)


@pytest.mark.parametrize("kind", ["flat", "pq", "sq"])
def test_array_folder_and_device_routes_build_one_index(kind, tmp_path):
    from clip_retrieval_amd import knn

    c = corpus()
    emb = str(tmp_path / "emb")
    os.makedirs(emb)
    np.save(os.path.join(emb, "img_emb_0.npy"), c["x"][:3000])
    np.save(os.path.join(emb, "img_emb_1.npy"), c["x"][3000:])
    built = {route: _build(kind, route, emb) for route in ("array", "folder", "device")}
    ref = built["array"]
    assert ref.ntotal == N and ref.nlist == NLIST and ref.nprobe == NLIST
    want = _codes(kind, ref)
    assert len(np.unique(want[-1])) > 1, "the rows all fell into one list"
    D0, I0 = ref.search(c["q"], 10)
    assert (I0 >= 0).all()
    for route in ("folder", "device"):
        got = _codes(kind, built[route])
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), f"{kind}: the {route} route's codes / lists differ from the array route's"
        D1, I1 = built[route].search(c["q"], 10)
        assert np.array_equal(I1, I0) and np.array_equal(D1.view(np.uint32), D0.view(np.uint32)), f"{kind}: {route} route searches differently"
    knn.save_index(built["array"], str(tmp_path / "a"), embeddings_folder=emb)
    knn.save_index(built["folder"], str(tmp_path / "f"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "f")) and any(n.endswith("manifest.json") for n in names)
    for n in names:
        if n.endswith("manifest.json"):
            assert _manifest_without_paths(tmp_path / "a" / n) == _manifest_without_paths(tmp_path / "f" / n), n
        else:
            assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "f" / n).read_bytes(), f"{kind}: {n} differs between the routes"
    for ix in built.values():
        ix.close()
