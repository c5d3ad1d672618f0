"""Indexes from disk and back ("img_emb_*.npy -> resident shards"; row a17: the reference builds once, offline --
clip_index.py:12-66 -- and boots by reading the index file -- clip_back.py:589-596, 883-896): save_index / load_index and the three
folder formats behind them.  IVF-Flat keeps centroids and list ids next to a manifest that names the embeddings (the arena is rebuilt
from them by one scatter pass); IVF-PQ and IVF-SQ8 folders are self-contained (codes, not rows) unless the PQ index has a refine store.
Every manifest is written last, so a folder without it is not an index.  Last of the kNN modules (knn_index <- knn_train <- knn_build
<- knn_store)."""

import glob
import json
import os

import numpy as np

from ._lib import check
from .knn_build import (FolderRows, _ivf_end, _ivfpq_begin, _ivfpq_encode_chunks, _ivfsq_begin, _positions_in_lists, _remember_folder,
                        _scatter_into_ivf)
from .knn_index import Mi355xIndex, ShardedMi355xIndex

IVF_MANIFEST = "ivf_manifest.json"
IVF_FORMAT = "clip-retrieval_amd ivf-flat v1"
IVFPQ_MANIFEST = "ivf_pq_manifest.json"
IVFPQ_ROTATION = "ivf_pq_rotation.npy"
IVFPQ_FORMAT = "clip-retrieval_amd ivf-pq v1"
IVFSQ_MANIFEST = "ivf_sq_manifest.json"
IVFSQ_FORMAT = "clip-retrieval_amd ivf-sq8 v1"


def _write_manifest(folder, name, man):
    """The manifest appears last and whole: written next to its place, then moved there.  Returns it."""
    tmp = os.path.join(folder, name + ".part")
    with open(tmp, "w", encoding="utf-8") as f:
        json.dump(man, f, indent=1)
    os.replace(tmp, os.path.join(folder, name))
    return man


def _read_manifest(folder, name):
    with open(os.path.join(folder, name), encoding="utf-8") as f:
        return json.load(f)


def threshold_scan_entry(on):
    """What a saved IVF-PQ or IVF-SQ8 manifest says about the threshold-scan switch: {"threshold_scan": true} when it is on, nothing
    otherwise."""
    return {"threshold_scan": True} if on else {}


def read_threshold_scan(folder, man):
    """The threshold-scan switch of a saved IVF-PQ or IVF-SQ8 manifest: False for a manifest without the key (every folder written
    before the switch existed, and every index saved with it off), else the boolean it carries; anything but a boolean is refused."""
    v = man.get("threshold_scan", False)
    if not isinstance(v, bool):
        raise ValueError(f"{folder}: \"threshold_scan\" must be true or false, got {v!r}")
    return v


ivfpq_threshold_scan_entry = ivfsq_threshold_scan_entry = threshold_scan_entry
read_ivfpq_threshold_scan = read_ivfsq_threshold_scan = read_threshold_scan


def _split_saved_rows(make, saved_range, nprobe, device, row_range, devices):
    """What load_index does with the saved rows [slo, shi) of an IVF index of any kind: all of them or `row_range` on one device, or
    an even split over `devices`.  make(lo, hi, device) builds one index over the rows [lo, hi) (global row numbers = ids)."""
    slo, shi = saved_range
    if devices is not None:
        if row_range is not None:
            raise ValueError("row_range and devices are mutually exclusive")
        G = len(devices)
        cuts = [slo + (shi - slo) * g // G for g in range(G + 1)]
        sharded = ShardedMi355xIndex.from_shards([make(cuts[g], cuts[g + 1], devices[g]) for g in range(G)], cuts[:-1])
        sharded.nprobe = nprobe
        return sharded
    lo, hi = (slo, shi) if row_range is None else (int(row_range[0]), int(row_range[1]))
    if not slo <= lo <= hi <= shi:
        raise ValueError(f"row_range {row_range} is outside the saved shard's rows [{slo}, {shi})")
    return make(lo, hi, device)


def _add_code_chunks(index, add_codes, codes, lists, lo, nlist, chunk, prepare=lambda c: c):
    """Saved codes (u8 [n, width], ids lo + row number) into an index between knnx_ivf_begin and knnx_ivf_end through the library's
    add_codes (knnx_ivfpq_add_codes / knnx_ivfsq_add_codes), `chunk` rows at a time."""
    lib = index._lib  # pylint: disable=protected-access
    cursor = np.zeros(nlist, dtype=np.int64)
    for o in range(0, codes.shape[0], chunk):
        c = np.ascontiguousarray(prepare(np.asarray(codes[o:o + chunk], dtype=np.uint8)))
        ls = np.ascontiguousarray(lists[o:o + chunk], dtype=np.int32)
        pos = _positions_in_lists(ls, cursor)
        ids = np.arange(lo + o, lo + o + c.shape[0], dtype=np.int64)
        check(lib, add_codes(index._h, c.ctypes.data, c.shape[0], ids.ctypes.data, ls.ctypes.data, pos.ctypes.data), "knnx")  # pylint: disable=protected-access


def load_index(path, device=0, row_range=None, enable_faiss_memory_mapping=False, devices=None, embeddings_folder=None):  # pylint: disable=unused-argument
    """Build an HBM-resident flat index from a folder of fp16 `.npy` partitions -- or, when `path` is a folder written by
    `save_index()` (it holds ivf_manifest.json), re-create that IVF-Flat index without training or assigning anything; a folder
    with ivf_pq_manifest.json / ivf_sq_manifest.json is read as that IVF-PQ / IVF-SQ8 index, straight from its saved codes.

    Takes the place of clip_back.py:589-596 (`faiss.read_index`) for this index type; ids are the global
    row order of the concatenated partitions = the metadata row order (clip_back.py:401-417).
    `row_range=(lo, hi)` loads one shard of a row-sharded index and sets its id base to `lo` (one process per GPU);
    `devices=[0, 1, ...]` builds ONE object that row-shards the whole folder over those GPUs of this process
    (`ShardedMi355xIndex`, the KnnService case).  `enable_faiss_memory_mapping` is accepted for call compatibility:
    rows are always resident in HBM; the files themselves are read through np.load(mmap_mode="r").
    """
    if os.path.isfile(os.path.join(path, IVFPQ_MANIFEST)):  # a saved IVF-PQ index: self-contained unless it has a refine store
        return _load_ivfpq_index(path, device=device, row_range=row_range, devices=devices, embeddings_folder=embeddings_folder)
    if os.path.isfile(os.path.join(path, IVFSQ_MANIFEST)):  # a saved IVF-SQ8 index: self-contained (codes, not rows)
        return _load_ivfsq_index(path, device=device, row_range=row_range, devices=devices)
    if os.path.isfile(os.path.join(path, IVF_MANIFEST)):  # a built IVF-Flat index saved by save_index(): no k-means, no assignment
        return _load_ivf_index(path, device=device, row_range=row_range, devices=devices)
    src = FolderRows(path)
    files, shapes, d, total = src.files, src.shapes, src.d, src.n
    lo, hi = (0, total) if row_range is None else row_range
    if devices is not None:
        if row_range is not None:
            raise ValueError("row_range and devices are mutually exclusive")
        index = ShardedMi355xIndex(d, devices)
        index.reserve(total)
    else:
        index = Mi355xIndex(d, device=device, id_base=lo)
        index.reserve(max(hi - lo, 0))
    start = 0
    for f, s in zip(files, shapes):
        a0, a1 = max(lo, start), min(hi, start + s[0])
        if a1 > a0:
            a = np.load(f, mmap_mode="r")[a0 - start:a1 - start]
            index.add(np.ascontiguousarray(a) if a.dtype in (np.float16, np.float32) else np.asarray(a, dtype=np.float32))
        start += s[0]
    return index


def save_index(index, folder, embeddings_folder=None):
    """Write a built IVF-Flat index (build_ivf_index_from_folder, or build_ivf_index given `embeddings_folder`) so that a service
    boots WITHOUT k-means or assignment: `ivf_centroids.npy` (fp16 [nlist, d]), `ivf_lists.npy` (int32 list id of every row of the
    shard: 4 bytes per row) and `ivf_manifest.json` (format, d, nlist, nprobe, row range, and the embeddings folder with the name
    and row count of each partition file -- the rows themselves are not copied: the arena is rebuilt from them by one scatter
    pass).  The counterpart of the reference's `<indices>/image.index` written by clip_index (clip_index.py:12-66), read back by
    `load_index(folder)` in the place of clip_back.py:589-596."""
    if getattr(index, "pq_m", 0):
        return _save_ivfpq_index(index, folder, embeddings_folder)
    if getattr(index, "is_sq", False):
        return _save_ivfsq_index(index, folder)
    lists, cent = getattr(index, "ivf_lists", None), getattr(index, "ivf_centroids", None)
    src = getattr(index, "ivf_source", None)
    if lists is None or cent is None:
        raise ValueError("save_index takes an IVF-Flat index built by build_ivf_index_from_folder / build_ivf_index")
    if src is None:
        if embeddings_folder is None:
            raise ValueError("this index was built from an in-memory array: name the embeddings folder its rows can be re-read from")
        src = FolderRows(embeddings_folder)
    lo, hi = getattr(index, "ivf_row_range", (0, src.n))
    if hi - lo != lists.shape[0]:
        raise ValueError("list ids and row range disagree")
    os.makedirs(folder, exist_ok=True)
    np.save(os.path.join(folder, "ivf_centroids.npy"), np.asarray(cent, dtype=np.float16))
    np.save(os.path.join(folder, "ivf_lists.npy"), np.asarray(lists, dtype=np.int32))
    return _write_manifest(folder, IVF_MANIFEST, {"format": IVF_FORMAT, "d": int(index.d), "nlist": int(cent.shape[0]), "nprobe": int(index.nprobe),
                                                  "row_range": [int(lo), int(hi)], **_embeddings_entries(src, folder)})


def _embeddings_entries(src, folder):
    """What a manifest in `folder` says about the embeddings folder `src`: its files, and where it is -- absolute and relative."""
    return {"embeddings": src.manifest(), "embeddings_relative": os.path.relpath(os.path.abspath(src.folder), os.path.abspath(folder))}


def read_ivf_manifest(folder, embeddings_folder=None):
    """(manifest dict, FolderRows of the embeddings it names) -- the embeddings are looked for at the recorded relative path
    first (the index folder and the embeddings usually move together), then at the absolute one; their file names and row
    counts must still be what they were when the index was built (ids are row numbers)."""
    man = _read_manifest(folder, IVF_MANIFEST)
    if man.get("format") != IVF_FORMAT:
        raise ValueError(f"{folder}: unknown index format {man.get('format')!r}")
    cands = [embeddings_folder] if embeddings_folder else [os.path.normpath(os.path.join(folder, man["embeddings_relative"])), man["embeddings"]["folder"]]
    src = None
    for c in cands:
        if c and os.path.isdir(c) and glob.glob(os.path.join(c, "*.npy")):
            src = FolderRows(c)
            break
    if src is None:
        raise FileNotFoundError(f"{folder}: the embeddings this index was built from are not at {cands}")
    if src.manifest()["files"] != man["embeddings"]["files"] or src.d != man["d"]:
        raise ValueError(f"{src.folder}: the embedding files changed since the index was built (names / row counts / dimension)")
    return man, src


def _load_ivf_index(folder, device=0, row_range=None, devices=None, embeddings_folder=None, chunk=1 << 20):
    man, src = read_ivf_manifest(folder, embeddings_folder)
    cent = np.load(os.path.join(folder, "ivf_centroids.npy"))
    lists = np.load(os.path.join(folder, "ivf_lists.npy"), mmap_mode="r")
    slo, shi = man["row_range"]
    if cent.shape != (man["nlist"], man["d"]) or lists.shape[0] != shi - slo:
        raise ValueError(f"{folder}: sidecar files disagree with the manifest")
    return _split_saved_rows(lambda lo, hi, dev: _scatter_into_ivf(src, lo, hi, cent, np.asarray(lists[lo - slo:hi - slo]), man["nprobe"], dev, chunk),
                             (slo, shi), man["nprobe"], device, row_range, devices)


def _save_ivfpq_index(index, folder, embeddings_folder=None):
    """The self-contained IVF-PQ folder: ivf_pq_centroids.npy (fp16 [nlist, d]), ivf_pq_codebooks.npy (f32 [M, 256, d_padded / M]),
    ivf_pq_codes.npy (u8 [n, M] in id order), ivf_pq_lists.npy (int32 [n]) and ivf_pq_manifest.json (written last); an index with an
    OPQ rotation adds ivf_pq_rotation.npy (f32 [d, d]) and "opq": true in the manifest; one whose quantiser space is wider than its
    rows also "d_out" (only then), and its rotation file is f32 [d_out, d], its centroids [nlist, d_out].  An index with a refine store adds "refine": true,
    "k_factor" and the embeddings folder (as save_index does for IVF-Flat) to the manifest: the rows are not written a second time, the
    folder is loaded together with the embeddings.  An index with the threshold scan switched on adds "threshold_scan": true (only
    then: every other folder is what it always was)."""
    cent = getattr(index, "ivf_centroids", None)
    if cent is None:
        raise ValueError("save_index takes an IVF-PQ index built by build_ivfpq_index* / load_index")
    src = None
    if index.pq_refine:
        src = embeddings_folder or getattr(index, "embeddings_folder", None)
        if src is None:
            raise ValueError("this IVF-PQ index has a refine store: name the embeddings folder its rows can be re-read from")
        src = src if isinstance(src, FolderRows) else FolderRows(src)
    codes, lists = index.pq_codes()
    lo, hi = getattr(index, "ivf_row_range", (0, codes.shape[0]))
    os.makedirs(folder, exist_ok=True)
    np.save(os.path.join(folder, "ivf_pq_centroids.npy"), np.asarray(cent, dtype=np.float16))
    np.save(os.path.join(folder, "ivf_pq_codebooks.npy"), index.pq_codebooks())
    np.save(os.path.join(folder, "ivf_pq_codes.npy"), codes)
    np.save(os.path.join(folder, "ivf_pq_lists.npy"), lists)
    man = {"format": IVFPQ_FORMAT, "d": int(index.d), "nlist": int(cent.shape[0]), "M": int(index.pq_m), "nprobe": int(index.nprobe),
           "row_range": [int(lo), int(hi)]}
    rot = index.pq_rotation()
    if rot is not None:  # (only then: a folder of an index without a rotation is what it always was)
        np.save(os.path.join(folder, IVFPQ_ROTATION), rot)
        man["opq"] = True
    man.update(ivfpq_out_dim_entry(index.d, index.pq_out_dim))
    if src is not None:
        if src.n < hi or src.d != index.d:
            raise ValueError(f"{src.folder}: {src.n} rows of width {src.d} cannot hold rows [{lo}, {hi}) of width {index.d}")
        man.update({"refine": True, "k_factor": int(index.k_factor), **_embeddings_entries(src, folder)})
    man.update(ivfpq_threshold_scan_entry(index.pq_threshold_scan))
    return _write_manifest(folder, IVFPQ_MANIFEST, man)


def ivfpq_out_dim_entry(d, d_out):
    """What a saved IVF-PQ manifest says about the quantiser width: {"d_out": d_out} when it differs from d, nothing otherwise."""
    return {"d_out": int(d_out)} if int(d_out) != int(d) else {}


def read_ivfpq_out_dim(folder, man):
    """The quantiser width of a saved IVF-PQ manifest: d for a manifest without "d_out" (every folder written before the key
    existed, and every index whose two widths agree), else the integer it carries -- which must obey the width rule and come with
    "opq": true, since only a rotation leads from d to d_out."""
    d = int(man["d"])
    if "d_out" not in man:
        return d
    v = man["d_out"]
    if not isinstance(v, int) or isinstance(v, bool) or v % 256 != 0 or d % 256 != 0 or not 256 <= d < v <= 1024:
        raise ValueError(f"{folder}: \"d_out\" must be a multiple of 256 with 256 <= d < d_out <= 1024 and d % 256 == 0, got d = {d}, "
                         f"d_out = {v!r}")
    if not man.get("opq", False):
        raise ValueError(f"{folder}: the manifest carries \"d_out\": {v} but does not say \"opq\": true (the rotation is what leads there)")
    return v


def read_ivfpq_rotation(folder, man):
    """The rotation a saved IVF-PQ folder carries: None for a manifest without "opq" (every folder written before the rotation
    existed), f32 [d, d] otherwise.  The flag and the file go together: either one without the other is refused.  A manifest with
    "d_out" carries f32 [d_out, d]; that shape is accepted only with the key, and the key only with that shape."""
    path = os.path.join(folder, IVFPQ_ROTATION)
    if not man.get("opq", False):
        if os.path.exists(path):
            raise ValueError(f"{folder}: {IVFPQ_ROTATION} is present but the manifest does not say \"opq\": true")
        if "d_out" in man:
            read_ivfpq_out_dim(folder, man)  # (raises: the key without the flag)
        return None
    if not os.path.isfile(path):
        raise ValueError(f"{folder}: the manifest says \"opq\": true but {IVFPQ_ROTATION} is missing")
    rot = np.load(path)
    d = int(man["d"])
    dq = read_ivfpq_out_dim(folder, man)
    if rot.shape != (dq, d) or rot.dtype != np.float32:
        raise ValueError(f"{folder}: {IVFPQ_ROTATION} must be float32 [{dq}, {d}], got {rot.dtype} {rot.shape}")
    return rot


def read_ivfpq_refine(folder, man, embeddings_folder=None):
    """The refine rules of a saved IVF-PQ manifest: (False, 1, None) for a manifest without "refine" (every folder written before the
    refine store existed, and every plain index since: self-contained), else (True, k_factor, FolderRows of the embeddings).  The
    embeddings are looked for at `embeddings_folder`, or at the recorded relative path, then at the absolute one; the flag without
    reachable embeddings, or embeddings whose files changed, are refused.  Touches no device."""
    if not man.get("refine", False):
        if "k_factor" in man:
            raise ValueError(f"{folder}: the manifest carries \"k_factor\" but does not say \"refine\": true")
        return False, 1, None
    kf = man.get("k_factor", 1)
    if not isinstance(kf, int) or isinstance(kf, bool) or not 1 <= kf <= 512:
        raise ValueError(f"{folder}: \"k_factor\" must be an integer in 1 .. 512, got {kf!r}")
    emb = man.get("embeddings")
    if not isinstance(emb, dict) or "files" not in emb:
        raise ValueError(f"{folder}: the manifest says \"refine\": true but names no embeddings")
    cands = [embeddings_folder] if embeddings_folder else [os.path.normpath(os.path.join(folder, man.get("embeddings_relative", "."))),
                                                            emb.get("folder")]
    src = None
    for c in cands:
        if c and os.path.isdir(c) and glob.glob(os.path.join(c, "*.npy")) and not os.path.isfile(os.path.join(c, IVFPQ_MANIFEST)):
            src = FolderRows(c)
            break
    if src is None:
        raise FileNotFoundError(f"{folder}: this IVF-PQ index has a refine store (\"refine\": true) and needs the embeddings it was built "
                                f"from; they are not at {cands} (pass embeddings_folder=)")
    if src.manifest()["files"] != emb["files"] or src.d != man["d"]:
        raise ValueError(f"{src.folder}: the embedding files changed since the index was built (names / row counts / dimension)")
    return True, kf, src


def _ivfpq_refine_from_rows(src, codes, lists, lo, cent, cb, M, nprobe, device, k_factor, chunk=1 << 20, rotation=None):
    """A saved refine index: rows [lo, lo + n) of the embeddings are stored AND re-encoded with the saved centroids, codebooks,
    rotation and lists; the codes that come out must be the saved ones."""
    n = codes.shape[0]
    index = _ivfpq_encode_chunks(((o - lo, x) for o, x in src.chunks(lo, lo + n, chunk)), n, src.d, cent.shape[0], M, cent, cb,
                                 np.asarray(lists, dtype=np.int32), nprobe, device, lo, rotation, True, k_factor)
    got = index.pq_codes()[0]
    if not np.array_equal(got, np.asarray(codes)):
        bad = int((got != np.asarray(codes)).any(axis=1).sum())
        index.close()
        raise ValueError(f"{bad} of {n} rows of {src.folder} do not encode to the saved ivf_pq_codes.npy: the embeddings or the codes changed")
    index.embeddings_folder = src.folder
    return _remember_folder(index, src)


def _ivfpq_from_codes(codes, lists, lo, cent, cb, M, nprobe, device, chunk=1 << 20, rotation=None):
    nlist, d = cent.shape
    if rotation is not None:  # (behind a rectangular rotation the centroids are d_out wide; the index is as wide as the rotation's input)
        d = rotation.shape[1]
    index = _ivfpq_begin(d, nlist, M, cent, cb, np.bincount(lists, minlength=nlist).astype(np.int64), device, lo, rotation)
    _add_code_chunks(index, index._lib.knnx_ivfpq_add_codes, codes, lists, lo, nlist, chunk)  # pylint: disable=protected-access
    return _ivf_end(index, nlist, nprobe, cent, lo, codes.shape[0], np.asarray(lists, dtype=np.int32))


def _load_ivfpq_index(folder, device=0, row_range=None, devices=None, embeddings_folder=None):
    man = _read_manifest(folder, IVFPQ_MANIFEST)
    if man.get("format") != IVFPQ_FORMAT:
        raise ValueError(f"{folder}: unknown index format {man.get('format')!r}")
    cent = np.load(os.path.join(folder, "ivf_pq_centroids.npy"))
    cb = np.load(os.path.join(folder, "ivf_pq_codebooks.npy"))
    codes = np.load(os.path.join(folder, "ivf_pq_codes.npy"), mmap_mode="r")
    lists = np.load(os.path.join(folder, "ivf_pq_lists.npy"), mmap_mode="r")
    rot = read_ivfpq_rotation(folder, man)
    refine, kf, src = read_ivfpq_refine(folder, man, embeddings_folder)
    thr_scan = read_ivfpq_threshold_scan(folder, man)
    slo, shi = man["row_range"]
    M = int(man["M"])

    def make(lo, hi, dev):
        c, ls = codes[lo - slo:hi - slo], np.asarray(lists[lo - slo:hi - slo])
        if refine:
            ix = _ivfpq_refine_from_rows(src, c, ls, lo, cent, cb, M, man["nprobe"], dev, kf, rotation=rot)
        else:
            ix = _ivfpq_from_codes(c, ls, lo, cent, cb, M, man["nprobe"], dev, rotation=rot)
        if thr_scan:
            ix.pq_threshold_scan = True
        return ix

    if cent.shape != (man["nlist"], read_ivfpq_out_dim(folder, man)) or codes.shape != (shi - slo, M) or lists.shape[0] != shi - slo:
        raise ValueError(f"{folder}: the IVF-PQ files disagree with the manifest")
    return _split_saved_rows(make, (slo, shi), man["nprobe"], device, row_range, devices)


def ivfsq_manifest(d, nlist, nprobe, row_range):
    """The manifest of a saved IVF-SQ8 folder (kind "ivfsq")."""
    return {"format": IVFSQ_FORMAT, "kind": "ivfsq", "d": int(d), "nlist": int(nlist), "nprobe": int(nprobe),
            "row_range": [int(row_range[0]), int(row_range[1])]}


def check_ivfsq_manifest(man, where=""):
    """A manifest read back: the format and the kind must be this one's, the numbers consistent.  Returns it."""
    if man.get("format") != IVFSQ_FORMAT or man.get("kind") != "ivfsq":
        raise ValueError(f"{where}: unknown index format {man.get('format')!r} / kind {man.get('kind')!r}")
    lo, hi = man["row_range"]
    if not (int(man["d"]) > 0 and int(man["nlist"]) > 0 and 0 <= int(lo) <= int(hi) and int(man["nprobe"]) >= 1):
        raise ValueError(f"{where}: inconsistent IVF-SQ8 manifest {man}")
    return man


def _save_ivfsq_index(index, folder):
    """The self-contained IVF-SQ8 folder: ivf_sq_centroids.npy (fp16 [nlist, d]), ivf_sq_vmin.npy / ivf_sq_vdiff.npy (f32 [d]),
    ivf_sq_codes.npy (u8 [n, d] in id order), ivf_sq_lists.npy (int32 [n]) and ivf_sq_manifest.json (kind "ivfsq", written last).  An
    index with the threshold scan switched on adds "threshold_scan": true (only then: other folders are byte-identical to before)."""
    cent = getattr(index, "ivf_centroids", None)
    if cent is None:
        raise ValueError("save_index takes an IVF-SQ8 index built by build_ivfsq_index* / load_index")
    codes, lists = index.sq_codes()
    vmin, vdiff = index.sq_quantizer()
    lo, hi = getattr(index, "ivf_row_range", (0, codes.shape[0]))
    os.makedirs(folder, exist_ok=True)
    np.save(os.path.join(folder, "ivf_sq_centroids.npy"), np.asarray(cent, dtype=np.float16))
    np.save(os.path.join(folder, "ivf_sq_vmin.npy"), vmin)
    np.save(os.path.join(folder, "ivf_sq_vdiff.npy"), vdiff)
    np.save(os.path.join(folder, "ivf_sq_codes.npy"), codes)
    np.save(os.path.join(folder, "ivf_sq_lists.npy"), lists)
    man = ivfsq_manifest(index.d, cent.shape[0], index.nprobe, (lo, hi))
    man.update(ivfsq_threshold_scan_entry(index.sq_threshold_scan))
    return _write_manifest(folder, IVFSQ_MANIFEST, man)


def _ivfsq_from_codes(codes, lists, lo, cent, ranges, nprobe, device, chunk=1 << 20, threshold_scan=False):
    nlist, d = cent.shape
    index = _ivfsq_begin(d, nlist, cent, ranges, np.bincount(lists, minlength=nlist).astype(np.int64), device, lo, threshold_scan)
    _add_code_chunks(index, index._lib.knnx_ivfsq_add_codes, codes, lists, lo, nlist, chunk, index._pad)  # pylint: disable=protected-access
    return _ivf_end(index, nlist, nprobe, cent, lo, codes.shape[0], np.asarray(lists, dtype=np.int32))


def _load_ivfsq_index(folder, device=0, row_range=None, devices=None):
    man = check_ivfsq_manifest(_read_manifest(folder, IVFSQ_MANIFEST), folder)
    thr_scan = read_ivfsq_threshold_scan(folder, man)
    cent = np.load(os.path.join(folder, "ivf_sq_centroids.npy"))
    ranges = (np.load(os.path.join(folder, "ivf_sq_vmin.npy")), np.load(os.path.join(folder, "ivf_sq_vdiff.npy")))
    codes = np.load(os.path.join(folder, "ivf_sq_codes.npy"), mmap_mode="r")
    lists = np.load(os.path.join(folder, "ivf_sq_lists.npy"), mmap_mode="r")
    slo, shi = man["row_range"]
    d = int(man["d"])
    if cent.shape != (man["nlist"], d) or codes.shape != (shi - slo, d) or lists.shape[0] != shi - slo or ranges[0].shape != (d,) or ranges[1].shape != (d,):
        raise ValueError(f"{folder}: the IVF-SQ8 files disagree with the manifest")
    return _split_saved_rows(lambda lo, hi, dev: _ivfsq_from_codes(codes[lo - slo:hi - slo], np.asarray(lists[lo - slo:hi - slo]), lo, cent, ranges,
                                                                   man["nprobe"], dev, threshold_scan=thr_scan),
                             (slo, shi), man["nprobe"], device, row_range, devices)
