"""The request hot path of `clip-retrieval back` on the MI355X index and encoder.

`KnnService` (clip_retrieval/clip_back.py:200-590) is a Flask resource; what it computes per request is
  compute_query  (:207-255)  text / image / embedding -> fp32 unit-norm query [1, d]
  knn_search     (:343-399)  index.search_and_reconstruct, post filter, ordered unique ids
  post filter    (:290-341)  near-duplicate removal (range search over the <= k result vectors), violence prompts, safety head
  map_to_metadata(:401-417)  metadata_provider.get(ids, cols) -> one record per result
`KnnHotPath` offers those four entry points with the reference's names, arguments and return values, so a maintainer binds them
onto KnnService.  The arithmetic is re-designed for the GPU rather than retyped:
  * dedup      k <= 64 (the client default is 40): fused into the coalesced search -- the result rows of every request of a batch are
               gathered once on the device and the links (normalised rows, inner product > 0.94, f32) of all of them come from one
               launch (knnx_search_dedup); larger k: one range scan of a resident GPU index over the result vectors -> CSR adjacency.
               Connected components on the host; a component keeps its best-ranked member (the reference's own DFS keeps the first
               node it visits, which is the smallest local index = the best rank);
  * violence   clip_back.py:327-331's einsum + argmax over the two prompt embeddings, the product in fp32 FMA on the GPU (the prompts
               as one resident bias-free Linear layer), argmax on the host (ties -> the smaller index, like np.argmax);
  * metadata   ids grouped by Arrow record batch, ONE `RecordBatch.take` per touched batch instead of a concat of 1-row slices per
               id (README.md:432: 41.5 ms); a single `Table.take` over chunked string columns measured 75 x slower;
  * safety     the H14 detector (h14_nsfw_model.py:16-34: seven fp32 Linear layers, ReLU between) runs on the GPU behind the
               reference's `.predict(embeddings, batch_size)` (`Mi355xSafetyHead`, csrc/postfilter.hip); any other object with
               `.predict` (the autokeras L/14 model) is called as the reference calls it.
Flask, prometheus and URL download stay where they are in the reference (out of scope).
"""

import ctypes as C
import os
import threading

import numpy as np

from ._lib import check, load_library
from .knn import Mi355xIndex


def normalized(a, axis=-1, order=2):
    """Rows scaled to unit norm, zero rows left alone (clip_back.py:194-197)."""
    n = np.atleast_1d(np.linalg.norm(a, order, axis))
    n[n == 0] = 1
    return a / np.expand_dims(n, axis)


class Mi355xSafetyHead:
    """Drop-in for `H14_NSFW_Detector` (clip_retrieval/h14_nsfw_model.py:10-50) in `clip_resource.safety_model`: the same
    `.predict(x, batch_size) -> float32 [n, out]`, computed on the GPU in fp32.

    state_dict: the detector's `layers.<i>.weight` / `layers.<i>.bias` tensors (numpy arrays or torch tensors), as saved in
    `<cache>/h14_nsfw_model/model.pt`.  The position numbers are those of its nn.Sequential (Linear, ReLU, Dropout, Linear, ...):
    a ReLU follows a Linear exactly when the next Linear does not sit at the very next position (positions 15 and 16 of the H14
    stack are back-to-back Linears, no activation between), never after the last one.  `relu=[...]` overrides."""

    def __init__(self, state_dict, device=0, relu=None):
        def arr(v):
            v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            return np.ascontiguousarray(v, dtype=np.float32)

        pos = sorted({int(k.split(".")[-2]) for k in state_dict if k.endswith(".weight")})
        if not pos:
            raise ValueError("no `<prefix>.<i>.weight` entries in the state dict")
        prefix = next(k for k in state_dict if k.endswith(f".{pos[0]}.weight"))[: -len(f"{pos[0]}.weight")]
        self._w = [arr(state_dict[f"{prefix}{i}.weight"]) for i in pos]
        self._b = [arr(state_dict[f"{prefix}{i}.bias"]) if f"{prefix}{i}.bias" in state_dict else None for i in pos]
        for a, b in zip(self._w[:-1], self._w[1:]):
            if a.ndim != 2 or b.ndim != 2 or b.shape[1] != a.shape[0]:
                raise ValueError(f"layer shapes do not chain: {a.shape} -> {b.shape}")
        if relu is None:
            relu = [j + 1 < len(pos) and pos[j + 1] != pos[j] + 1 for j in range(len(pos))]
        self.relu = [bool(r) for r in relu]
        self.dims = [self._w[0].shape[1]] + [w.shape[0] for w in self._w]
        self.input_size = self.dims[0]
        self.device = int(device)  # where the layers live: Mi355xIndex.search_filtered runs them only beside an index of that device
        self._lib = load_library()
        n = len(pos)
        dims = (C.c_int32 * (n + 1))(*self.dims)
        wp = (C.c_void_p * n)(*[w.ctypes.data for w in self._w])
        bp = (C.c_void_p * n)(*[b.ctypes.data if b is not None else None for b in self._b])
        rl = (C.c_uint8 * n)(*[1 if r else 0 for r in self.relu])
        h = C.c_void_p()
        check(self._lib, self._lib.knnx_mlp_create(int(device), n, dims, wp, bp, rl, C.byref(h)), "knnx")
        self._h = h

    @classmethod
    def from_cache(cls, cache_folder=os.path.expanduser("~/.cache/clip_retrieval"), device=0):
        """The reference's file location (h14_nsfw_model.py:58-72); no download here: the file has to be there."""
        import torch  # pylint: disable=import-outside-toplevel

        path = os.path.join(cache_folder, "h14_nsfw_model", "model.pt")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path}: the H14 detector's weights are not cached (the reference downloads h14_nsfw.pth there)")
        return cls(torch.load(path, map_location="cpu"), device=device)

    def predict(self, x, batch_size=None):  # pylint: disable=unused-argument
        x = np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.dims[0]:
            raise ValueError(f"expected [n, {self.dims[0]}] inputs, got {x.shape}")
        y = np.empty((x.shape[0], self.dims[-1]), dtype=np.float32)
        check(self._lib, self._lib.knnx_mlp_forward(self._h, x.ctypes.data, x.shape[0], y.ctypes.data), "knnx")
        return y

    def close(self):
        if getattr(self, "_h", None):
            self._lib.knnx_mlp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass


class ArrowMetadataProvider:
    """Metadata of contiguous ids from memory-mapped Arrow IPC files (clip_back.py:599-615).  Same constructor, same
    `get(ids, cols) -> list of dict records`, same row order (the order of `ids`, duplicates kept), same column filter (unknown
    columns are ignored).  The reference concatenates one 1-row slice of the whole table per id; here the ids are grouped by the
    record batch they fall into (one searchsorted over the batch offsets), every touched batch is asked ONCE for its rows
    (`RecordBatch.take`: O(rows taken), memory-mapped pages of the touched rows only) and the pieces are put back into request
    order.  (`Table.take` over the chunked table is NOT this: pyarrow flattens string chunks first -- measured 33 ms per request
    on a 10 M-row table against 0.4 ms for the reference's slicing at k = 40, profiles/r03b_request.log.)"""

    def __init__(self, arrow_folder):
        from pathlib import Path  # pylint: disable=import-outside-toplevel

        import pyarrow as pa  # pylint: disable=import-outside-toplevel

        files = [str(a) for a in sorted(Path(arrow_folder).glob("**/*")) if a.is_file()]
        self.table = pa.concat_tables([pa.ipc.RecordBatchFileReader(pa.memory_map(f, "r")).read_all() for f in files])
        self._batches = self.table.to_batches()
        self._starts = np.cumsum([0] + [b.num_rows for b in self._batches])

    def get(self, ids, cols=None):
        import pyarrow as pa  # pylint: disable=import-outside-toplevel

        names = self.table.schema.names
        cols = names if cols is None else [c for c in names if c in set(cols)]
        ids = np.asarray(list(ids), dtype=np.int64)
        if ids.size == 0:
            return []
        if ids.min() < 0 or ids.max() >= self._starts[-1]:
            raise IndexError(f"metadata id out of range [0, {int(self._starts[-1])})")
        which = np.searchsorted(self._starts, ids, side="right") - 1
        order = np.argsort(which, kind="stable")
        pieces, pos = [], 0
        sorted_which = which[order]
        while pos < len(order):
            b = int(sorted_which[pos])
            end = int(np.searchsorted(sorted_which, b, side="right"))
            local = ids[order[pos:end]] - self._starts[b]
            pieces.append(self._batches[b].select(cols).take(pa.array(local)))
            pos = end
        rows = pa.Table.from_batches(pieces).to_pylist()  # in `order`; hand them back in request order
        out = [None] * len(ids)
        for r, o in zip(rows, order):
            out[int(o)] = r
        return out


IVF_MAPPING_FILE = "ivf_old_to_new_mapping.npy"


def load_ivf_old_to_new_mapping(indice_folder, image_index):
    """The reference's file protocol for the id mapping of a metadata store ordered by inverted list (clip_back.py:629-640):
    `<indice_folder>/ivf_old_to_new_mapping.npy` is, despite its name, a RAW int64 memmap without an npy header.  It is written once
    when absent -- from `image_index.ivf_old_to_new()`, one pass on the device -- and memory-mapped read-only from then on; a file the
    reference wrote loads here and the reverse.  The result goes into `clip_resource.ivf_old_to_new_mapping`; a service may also leave
    that None and let KnnHotPath translate through `image_index.map_ids` without any per-row table on the host."""
    path = os.path.join(indice_folder, IVF_MAPPING_FILE)
    if not os.path.exists(path):
        mapping = np.ascontiguousarray(image_index.ivf_old_to_new(), dtype=np.int64)
        tmp = path + ".tmp"  # (never a half-written file under the final name)
        out = np.memmap(tmp, dtype="int64", mode="w+", shape=mapping.shape)
        out[:] = mapping
        out.flush()
        del out
        os.replace(tmp, path)
    return np.memmap(path, dtype="int64", mode="r")


def reorder_arrow_metadata(index, src_folder, dst_folder, columns=None, rows_per_file=1 << 20):
    """Write the Arrow IPC metadata of `src_folder` (what ArrowMetadataProvider reads: row i = id i) into `dst_folder` ordered by the
    inverted lists of `index`: row o of the result is source row new_to_old[o], so that
    `ArrowMetadataProvider(dst_folder).get(index.map_ids(ids)) == ArrowMetadataProvider(src_folder).get(ids)` and the results of one
    probed list are one contiguous run.  Streams: every output file (`rows_per_file` rows, one record batch) is gathered from the
    memory-mapped source batches it touches and written before the next one is looked at; the table is never materialised.  `columns`
    keeps a subset (unknown names are ignored, like the provider's filter).  Returns the files written.  (The reference's HDF5 sink --
    ivf_metadata_ordering.py:87-131 -- is out of scope: DESIGN section 7.)"""
    from pathlib import Path  # pylint: disable=import-outside-toplevel

    import pyarrow as pa  # pylint: disable=import-outside-toplevel

    files = [str(a) for a in sorted(Path(src_folder).glob("**/*")) if a.is_file()]
    if not files:
        raise ValueError(f"no Arrow files under {src_folder}")
    readers = [pa.ipc.RecordBatchFileReader(pa.memory_map(f, "r")) for f in files]
    where = [(r, b) for r in readers for b in range(r.num_record_batches)]  # global batch number -> (reader, batch in it)
    schema = readers[0].schema
    names = schema.names if columns is None else [c for c in schema.names if c in set(columns)]
    out_schema = pa.schema([schema.field(c) for c in names])
    starts = np.cumsum([0] + [r.get_batch(b).num_rows for r, b in where])
    new_to_old = np.asarray(index.ivf_new_to_old(), dtype=np.int64)
    if int(starts[-1]) != new_to_old.shape[0]:
        raise ValueError(f"{src_folder} holds {int(starts[-1])} rows, the index {new_to_old.shape[0]}")
    id_base = int(new_to_old.min()) if new_to_old.size else 0
    if id_base != 0:
        raise ValueError(f"the index's ids start at {id_base}: metadata rows are addressed by ids from 0 (map a sharded index as a whole)")
    rows_per_file = max(int(rows_per_file), 1)
    os.makedirs(dst_folder, exist_ok=True)
    written = []
    for part, lo in enumerate(range(0, new_to_old.shape[0], rows_per_file)):
        src = new_to_old[lo:lo + rows_per_file]
        which = np.searchsorted(starts, src, side="right") - 1
        order = np.argsort(which, kind="stable")
        sorted_which = which[order]
        pieces, pos = [], 0
        while pos < len(order):  # one take per source batch this file touches (ArrowMetadataProvider.get does the same per request)
            b = int(sorted_which[pos])
            end = int(np.searchsorted(sorted_which, b, side="right"))
            r, bi = where[b]
            pieces.append(r.get_batch(bi).select(names).take(pa.array(src[order[pos:end]] - starts[b])))
            pos = end
        back = np.empty(len(order), dtype=np.int64)
        back[order] = np.arange(len(order))  # the pieces are in `order`; put the rows back into list order
        table = pa.Table.from_batches(pieces, schema=out_schema).take(pa.array(back)).combine_chunks()
        if part > 99999:  # (the provider reads the files in name order: five digits keep that the part order)
            raise ValueError("more than 100 000 output files: raise rows_per_file")
        path = os.path.join(dst_folder, f"{part:05d}.arrow")
        with pa.OSFile(path, "wb") as sink, pa.ipc.new_file(sink, out_schema) as writer:
            for batch in table.to_batches():
                writer.write_batch(batch)
        written.append(path)
    return written


class _ResidentIndexPool:
    """Small flat GPU indexes that live as long as the service (allocating one per request would cost more than the search),
    a few per embedding width so that concurrent request threads (clip_back.py:1018) do not queue behind ONE dedup index:
    `borrow(rows)` yields an index refilled with `rows`."""

    def __init__(self, device, size=8):
        import queue  # pylint: disable=import-outside-toplevel

        self._device, self._size = device, size
        self._free = {}     # d -> queue of idle indexes
        self._made = {}     # d -> number created so far
        self._lock = threading.Lock()
        self._queue = queue.Queue

    def borrow(self, rows):
        import contextlib  # pylint: disable=import-outside-toplevel

        d = rows.shape[1]
        with self._lock:
            q = self._free.setdefault(d, self._queue())
            make = q.empty() and self._made.get(d, 0) < self._size
            if make:
                self._made[d] = self._made.get(d, 0) + 1
        if make:
            try:
                ix = Mi355xIndex(d, device=self._device, coalesce=False)
            except BaseException:
                with self._lock:  # a failed construction must not use up one of the pool's `size` places for good (ADVICE r3:
                    self._made[d] -= 1  # after `size` failures every later request would block forever in q.get())
                raise
        else:
            ix = q.get()

        @contextlib.contextmanager
        def lease():
            try:
                ix.reset()
                ix.add(rows)
                yield ix
            finally:
                q.put(ix)

        return lease()


class KnnHotPath:
    """The arithmetic of one /knn-service request.  `clip_resource` is the reference's ClipResource-shaped object:
    .model / .tokenizer / .preprocess (encoder.load_clip), .image_index / .text_index (knn.Mi355xIndex or
    knn.ShardedMi355xIndex), .safety_model, .violence_detector, .aesthetic_embeddings, .metadata_is_ordered_by_ivf and
    .ivf_old_to_new_mapping (None: the image index translates the ids itself)."""

    def __init__(self, dedup_device=0, device_filter=False):
        # device_filter: large-k requests (and small ones with a safety / violence filter) run their whole post filter beside the index
        # (Mi355xIndex.search_filtered) when the index offers it and every active model is a device head there; off: knn_search is
        # the general path below, line for line
        self._device_filter = bool(device_filter)
        self._scratch = _ResidentIndexPool(dedup_device)   # dedup: the request's own result vectors
        self._prompts = {}                             # (shape, content hash) -> (the prompt array, its resident fp32 Linear layer)
        self._prompts_lock = threading.Lock()
        self._nprobe_lock = threading.Lock()
        self._device = dedup_device

    # ------------------------------------------------------------------ clip_back.py:207-255
    def compute_query(self, clip_resource, text_input, image_input, image_url_input, embedding_input, use_mclip=False,
                      aesthetic_score=None, aesthetic_weight=None):
        """fp32 [1, d] query.  Exactly one of the inputs is used, in the reference's order of precedence."""
        feats = query = None
        if text_input and use_mclip:
            # clip_back.py:222-224: the multilingual tower's own callable (mclip.load_mclip), normalised in numpy, float32
            fn = getattr(clip_resource, "model_txt_mclip", None)
            if fn is None:
                raise NotImplementedError("use_mclip was requested but the clip resource has no model_txt_mclip (mclip.load_mclip)")
            query = np.asarray(normalized(np.asarray(fn(text_input), dtype=np.float32)), dtype=np.float32).reshape(1, -1)
        elif text_input:
            feats = clip_resource.model.encode_text(clip_resource.tokenizer([text_input]))
        elif image_input is not None:
            import base64  # pylint: disable=import-outside-toplevel
            from io import BytesIO  # pylint: disable=import-outside-toplevel

            from PIL import Image  # pylint: disable=import-outside-toplevel

            pixels = clip_resource.preprocess(Image.open(BytesIO(base64.b64decode(image_input))))
            feats = clip_resource.model.encode_image(pixels.unsqueeze(0))
        elif image_url_input is not None:
            raise NotImplementedError("image_url_input needs the reference's download_image (networking: out of scope)")
        if feats is not None:
            # the encoder already returns unit-norm fp32 rows; dividing again keeps the reference's exact contract for any model
            query = (feats / feats.norm(dim=-1, keepdim=True)).cpu().float().numpy()
        elif query is None and embedding_input is not None:
            query = np.asarray(embedding_input, dtype=np.float32)[None, :]
        elif query is None:
            return None
        aest = getattr(clip_resource, "aesthetic_embeddings", None)
        if aest is not None and aesthetic_score is not None:
            query = query + aest[aesthetic_score] * aesthetic_weight
            query = query / np.linalg.norm(query)
        return query

    # ------------------------------------------------------------------ clip_back.py:290-309 (+ :270-288)
    def get_non_uniques(self, embeddings, threshold=0.94):
        """Local indices of the results that duplicate a better-ranked one: rows whose inner product exceeds `threshold` are
        linked; of every connected group only the smallest index (= best rank) survives."""
        embeddings = np.ascontiguousarray(embeddings, dtype=np.float32)
        n = embeddings.shape[0]
        if n == 0:
            return []
        with self._scratch.borrow(embeddings) as ix:
            lims, _, nbr = ix.range_search(embeddings, threshold)
        return self.non_uniques_from_links(lims, nbr, n)

    @staticmethod
    def non_uniques_from_links(lims, nbr, n):
        """Range-search result in CSR form (row i links to nbr[lims[i]:lims[i+1]]) -> every node that is not the smallest
        index of its connected group."""
        from scipy.sparse import csr_matrix  # pylint: disable=import-outside-toplevel
        from scipy.sparse.csgraph import connected_components  # pylint: disable=import-outside-toplevel

        lims, nbr = np.asarray(lims), np.asarray(nbr)
        if len(nbr) <= n and np.array_equal(nbr, np.flatnonzero(np.diff(lims) == 1)):
            return []  # the common request: every row is linked to itself at most -- nothing to group
        graph = csr_matrix((np.ones(len(nbr), dtype=np.int8), nbr, lims), shape=(n, n))
        _, label = connected_components(graph, directed=False)
        first = np.full(label.max() + 1, n, dtype=np.int64)
        np.minimum.at(first, label, np.arange(n))
        return np.flatnonzero(first[label] != np.arange(n)).tolist()

    @staticmethod
    def non_uniques_from_pairs(pairs, n):
        """Links (i, j) between result ranks -> every rank that is not the smallest of its connected group (the reference keeps
        g[0] of every component, and its components start from the smallest unseen node: clip_back.py:270-288, 303-307)."""
        if len(pairs) == 0:
            return []
        parent = list(range(n))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a

        for i, j in pairs:
            a, b = find(int(i)), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)  # the root of a group is its smallest member
        return [i for i in range(n) if find(i) != i]

    connected_components_dedup = get_non_uniques

    # ------------------------------------------------------------------ clip_back.py:315-341
    @staticmethod
    def get_unsafe_items(safety_model, embeddings, threshold=0.5):
        """Indices the safety head scores above `threshold` (the model is the reference's: anything with `.predict`)."""
        scores = np.asarray(safety_model.predict(embeddings, batch_size=embeddings.shape[0]))
        return np.flatnonzero(scores.reshape(len(scores), -1)[:, 0] > threshold)

    def get_violent_items(self, safety_prompts, embeddings):
        """Indices whose best-matching prompt is prompt 1 ("violent"): clip_back.py:327-331's
        `argmax(einsum("ij,kj->ik", embeddings, safety_prompts), axis=1) == 1`, the product in fp32 FMA on the GPU (one bias-free
        Linear layer of csrc/postfilter.hip; the prompt matrix stays resident IN FP32 -- round 3 kept it as a 2-row fp16 index,
        whose rounding could flip a near-tie against the reference's fp32 einsum).  The resident copy is keyed on the
        array's CONTENT and holds a reference to it (an id() can be reused by a new array); the GPU call runs outside the lock."""
        embeddings = np.ascontiguousarray(embeddings, dtype=np.float32)
        if embeddings.shape[0] == 0:
            return np.zeros(0, dtype=np.int64)
        scores = self._prompt_head(safety_prompts).predict(embeddings, batch_size=embeddings.shape[0])
        return np.flatnonzero(np.argmax(scores, axis=1) == 1)

    def _prompt_head(self, safety_prompts):
        """The resident bias-free Linear layer over the violence prompts (cached by content; see get_violent_items)."""
        prompts = np.ascontiguousarray(safety_prompts, dtype=np.float32)
        key = (prompts.shape, hash(prompts.tobytes()))
        with self._prompts_lock:
            hit = self._prompts.get(key)
            if hit is None or not np.array_equal(hit[0], prompts):
                if len(self._prompts) >= 8:  # a service has one detector; do not grow without bound if a caller keeps swapping it
                    self._prompts.clear()
                hit = self._prompts[key] = (prompts, Mi355xSafetyHead({"layers.0.weight": prompts}, device=self._device, relu=[False]))
        return hit[1]

    def post_filter(self, safety_model, embeddings, deduplicate, use_safety_model, use_violence_detector, violence_detector):
        """Local indices to drop: duplicates | violent | unsafe."""
        drop = set()
        if deduplicate:
            drop.update(self.get_non_uniques(embeddings))
        if use_violence_detector and violence_detector is not None:
            drop.update(int(i) for i in self.get_violent_items(violence_detector, embeddings))
        if use_safety_model and safety_model is not None:
            drop.update(int(i) for i in self.get_unsafe_items(safety_model, embeddings))
        return drop

    # ------------------------------------------------------------------ clip_back.py:343-399
    def knn_search(self, query, modality, num_result_ids, clip_resource, deduplicate, use_safety_model, use_violence_detector):
        """(distances, indices): the index's answer cut at the first -1, minus the post filter's picks, each id once, best
        first.  With `clip_resource.metadata_is_ordered_by_ivf` the surviving ids are translated into the ids of the list-ordered
        metadata store as the last step (_ivf_id_mapper).
        An IVF-PQ index serves num_result_ids <= 64 as it stands; the Python default of 100, the front end's 3 000 and the >= 100 000
        requests of the probe-widening branch below need its threshold scan switched on (Mi355xIndex.pq_threshold_scan, or
        threshold_scan=True at build time; saved with the index) -- without it the index answers them with KNNX_E_UNSUPPORTED, which
        is raised, never papered over.  An IVF-SQ8 index has the same rule and its own switch (Mi355xIndex.sq_threshold_scan).  No
        branch of this function depends on either switch."""
        to_new = self._ivf_id_mapper(clip_resource)
        index = clip_resource.image_index if modality == "image" else clip_resource.text_index
        # clip_back.py:356-369: a request for >= 100 000 results widens the IVF probe to ceil(k / 3000) lists for the duration of the
        # search (nprobe lists hold ~nprobe * N / nlist rows: fewer than k otherwise) and puts the old value back.  The reference does
        # this on its IVF-reordered branch; here it applies to every IVF-Flat index.  nprobe is index-wide state, so such requests
        # are serialised among themselves (the reference has the same race and no lock).
        wide = num_result_ids >= 100000 and getattr(index, "nlist", 0) > 0
        safety_model = getattr(clip_resource, "safety_model", None)
        violence_detector = getattr(clip_resource, "violence_detector", None)
        need_vectors = (use_safety_model and safety_model is not None) or (use_violence_detector and violence_detector is not None)
        query = np.asarray(query)
        links = None
        if getattr(self, "_device_filter", False) and not wide:  # (getattr: a hot path made without __init__ has no switch, so it is off)
            answer = self._knn_search_device_filter(index, query, num_result_ids, to_new, deduplicate,
                                                    safety_model if use_safety_model else None,
                                                    violence_detector if use_violence_detector else None)
            if answer is not None:
                return answer
        if wide:
            import math  # pylint: disable=import-outside-toplevel

            with self._nprobe_lock:
                previous = index.nprobe
                index.nprobe = min(index.nlist, max(previous, math.ceil(num_result_ids / 3000)))
                try:
                    D, I, R = index.search_and_reconstruct(query, num_result_ids)
                finally:
                    index.nprobe = previous
        elif deduplicate and num_result_ids <= 64 and query.shape[0] == 1 and hasattr(index, "search_dedup"):
            # the request's dedup fused into the coalesced search (knnx_search_dedup): the k result rows are gathered once on the
            # device for every request of the batch, the links of all of them come from one launch, and the rows only travel to
            # the host when another filter needs them
            D, I, R, links = index.search_dedup(query, num_result_ids, 0.94, want_r=need_vectors)
            if links is None and R is None:  # more links than the device keeps: the general path below
                R = index.reconstruct_batch(I[0])[None]
        elif deduplicate or need_vectors:
            D, I, R = index.search_and_reconstruct(query, num_result_ids)
        else:
            D, I = index.search(query, num_result_ids)  # no filter looks at the vectors: they stay in HBM
            R = None
        ids = I[0]
        ids_l = ids.tolist() if len(ids) <= 4096 else None  # small answers (the client default is 40): plain Python beats numpy calls
        if ids_l is not None:
            n = ids_l.index(-1) if ids_l[-1] == -1 else len(ids_l)
        else:
            n = int(np.argmax(ids == -1)) if (ids == -1).any() else len(ids)
        ids, dist = ids[:n], D[0][:n]
        if (ids_l is not None and not need_vectors and (not deduplicate or (links is not None and len(links) == 0))
                and len(set(ids_l[:n])) == n):
            # nothing to drop, every id once: the answer as it is (numpy scalars, like the reference's lists)
            return list(dist), list(ids if to_new is None else to_new(ids))
        keep = np.ones(n, dtype=bool)
        drop = set()
        emb = normalized(R[0][:n]) if R is not None else None
        if deduplicate:
            if links is not None:
                links = links[(links[:, 0] < n) & (links[:, 1] < n)]
                drop.update(self.non_uniques_from_pairs(links, n))
            else:
                drop.update(self.get_non_uniques(emb))
        if need_vectors:
            drop.update(self.post_filter(safety_model, emb, False, use_safety_model, use_violence_detector, violence_detector))
        if drop:
            keep &= ~np.isin(ids, ids[np.fromiter(drop, dtype=np.int64)])  # an id the filter dropped goes everywhere it occurs
        _, first = np.unique(ids, return_index=True)                       # an id is reported once, at its best rank
        once = np.zeros(n, dtype=bool)
        once[first] = True
        sel = np.flatnonzero(keep & once)
        return list(dist[sel]), list(ids[sel] if to_new is None else to_new(ids[sel]))

    def _knn_search_device_filter(self, index, query, k, to_new, deduplicate, safety_model, violence_detector):
        """knn_search through Mi355xIndex.search_filtered, or None where the request is the general path's: nothing to filter at k <= 64
        (the fused dedup serves that), k above the device filter's limit, an index without the method (ShardedMi355xIndex), or an
        active model that is not a device head on the index's device.  Behind the drop bytes the assembly is the general path's: cut at
        -1, an id the filter dropped goes everywhere it occurs, each id once, to_new.  A request with more links than the device keeps
        re-runs dedup alone through reconstruct_batch + get_non_uniques."""
        need_vectors = safety_model is not None or violence_detector is not None
        if not (deduplicate or need_vectors) or not (k > 64 or need_vectors) or k > 8192 or query.shape[0] != 1:
            return None
        if not hasattr(index, "search_filtered"):
            return None
        if safety_model is not None and not (isinstance(safety_model, Mi355xSafetyHead) and safety_model.device == index.device):
            return None
        violence = None
        if violence_detector is not None:
            violence = self._prompt_head(violence_detector)
            if violence.device != index.device:
                return None
        D, I, bits, stats = index.search_filtered(query, k, 0.94 if deduplicate else None, violence, safety_model, 0.5)
        ids = I[0]
        n = int(np.argmax(ids == -1)) if (ids == -1).any() else len(ids)
        ids, dist = ids[:n], D[0][:n]
        drop = set(np.flatnonzero(bits[:n]).tolist())
        if deduplicate and stats["links_overflowed"]:
            drop.update(self.get_non_uniques(normalized(index.reconstruct_batch(ids))))
        keep = np.ones(n, dtype=bool)
        if drop:
            keep &= ~np.isin(ids, ids[np.fromiter(drop, dtype=np.int64)])  # an id the filter dropped goes everywhere it occurs
        _, first = np.unique(ids, return_index=True)                       # an id is reported once, at its best rank
        once = np.zeros(n, dtype=bool)
        once[first] = True
        sel = np.flatnonzero(keep & once)
        return list(dist[sel]), list(ids[sel] if to_new is None else to_new(ids[sel]))

    @staticmethod
    def _ivf_id_mapper(clip_resource):
        """None, or -- with `metadata_is_ordered_by_ivf` -- the translation of result ids into the ids of a metadata store ordered by
        inverted list (clip_back.py:350-364).  The search runs exactly as without it; the ids that survive the cut at -1 and the post
        filter are translated last, so the fewest ids travel and -1 never reaches the mapping.  The mapping is ALWAYS the image
        index's, whichever index was searched: the metadata is ordered by the image index's lists, and the reference maps text
        results through the same array.  `clip_resource.ivf_old_to_new_mapping` (the reference's array; works with any index object)
        wins when it is not None, otherwise `image_index.map_ids` translates on the device without a per-row table on the host."""
        if not getattr(clip_resource, "metadata_is_ordered_by_ivf", False):
            return None
        table = getattr(clip_resource, "ivf_old_to_new_mapping", None)
        if table is not None:
            return lambda ids: np.take(table, ids)
        mapper = clip_resource.image_index.map_ids
        return lambda ids: mapper(np.ascontiguousarray(ids, dtype=np.int64))

    # ------------------------------------------------------------------ clip_back.py:401-417
    @staticmethod
    def map_to_metadata(indices, distances, num_images, metadata_provider, columns_to_return):
        """One record per result: the metadata columns of the first `num_images` ids (bytes decoded as utf-8) + id + similarity."""
        metas = metadata_provider.get(indices[:num_images], columns_to_return)
        out = []
        for rank, (d, i) in enumerate(zip(distances, indices)):
            rec = {}
            if rank < len(metas) and metas[rank] is not None:
                rec.update((k, v.decode("utf-8") if isinstance(v, bytes) else v) for k, v in metas[rank].items())
            rec["id"] = i.item() if hasattr(i, "item") else int(i)
            rec["similarity"] = d.item() if hasattr(d, "item") else float(d)
            out.append(rec)
        return out
