#!/usr/bin/env python3
"""One /knn-service request, measured stage by stage (README.md:429-437 publishes the reference's stage means:
text clip inference 18.6 ms, image 20.6 ms, knn index 26.7 ms, metadata get 41.5 ms on its CPU box).

    python tools/request_bench.py [--rows 100000000 --meta-rows 10000000 --reps 20]

A request = KnnHotPath.compute_query -> knn_search (search_and_reconstruct + post filter) -> map_to_metadata
(clip_back.py:419-470).  Encoder: ViT-L/14 (random-init weights, synthetic BPE vocabulary: neither the checkpoint nor the
vocabulary file exists offline -- the arithmetic per request is the same); index: flat IP over --rows x 768 fp16 rows resident
in HBM (BASELINE config 3); metadata: an Arrow IPC table of --meta-rows rows (url, caption), memory-mapped, through the
reference's per-id slicing (clip_back.py:608-615 restated) and through service.ArrowMetadataProvider's batched take.
Prints a table like README.md:429-437 and one JSON line (prefix "REQUEST ").

    python tools/request_bench.py --serve-threads 64 [--ordered-by-ivf] [--ivf-rows 16777216 --nlist 16384 --requests 200]

The serving side alone: --serve-threads request threads, each sending one-query requests (knn_search at k = 40 + map_to_metadata) to ONE
IVF-PQ index built on the device, as clip_back's werkzeug threads do.  --ordered-by-ivf serves the same request stream with
metadata_is_ordered_by_ivf=True: the ids are translated by the image index (Mi355xIndex.map_ids) and the metadata comes from a folder
re-ordered by its lists.  Prints one JSON line (prefix "SERVE ").

    python tools/request_bench.py --device-filter [--filter-index flat|ivfsq --rows N --ivf-rows N --nlist L --nprobe P --rounds 5 --reps 10]
                                  [--serve-threads 64 --requests 20]

The post filter of knn_search where the rows are (KnnHotPath(device_filter=True) -> Mi355xIndex.search_filtered) against the general path
(the switch off: search_and_reconstruct + host normalisation + scratch-index dedup + the heads over host rows), in ONE process on ONE
index: a flat --rows x 768 index or an IVF-SQ8 --ivf-rows x 1024 index with its threshold scan on, safety (H14-shaped, random weights)
and violence models in the clip_resource.  k = 40 and 3 000, dedup alone and all three filters; --rounds rounds, the two switch
positions alternating inside each round, --reps requests per position; per position the median request of every round, then the median
and the spread (min .. max) of the round medians.  With --serve-threads T a further leg, labelled as such: T threads x --requests
requests at k = 3 000 with all three filters, switch off then on.  Prints one JSON line per leg (prefix "FILTER ").
"""
import argparse
import base64
import gzip
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_merges(folder):
    from clip_retrieval_amd.tokenizer import BPE_FILE_NAME, bytes_to_unicode

    b2u = bytes_to_unicode()
    merges, seen = [], set()
    for w in "a photo of the cat dog red blue car house tree sky person walking on beach in city at night".split():
        sym = [b2u[b] for b in w.encode()]
        sym[-1] += "</w>"
        while len(sym) > 1:
            p = (sym[0], sym[1])
            if p not in seen:
                seen.add(p)
                merges.append(p)
            sym = [sym[0] + sym[1]] + sym[2:]
    with gzip.open(os.path.join(folder, BPE_FILE_NAME), "wt", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(" ".join(m) for m in merges) + "\n")


class ReferenceStyleProvider:
    """clip_back.py:599-615 restated: one 1-row slice per id, concatenated (what the batched take replaces)."""

    def __init__(self, table):
        self.table = table

    def get(self, ids, cols=None):
        import pyarrow as pa

        if cols is None:
            cols = self.table.schema.names
        else:
            cols = list(set(self.table.schema.names) & set(cols))
        t = pa.concat_tables([self.table[i:i + 1] for i in ids])
        return t.select(cols).to_pandas().to_dict("records")


def serve(a):
    """--serve-threads: requests per second of the search + metadata half under concurrent one-query callers."""
    import threading
    from types import SimpleNamespace

    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    import torch

    from clip_retrieval_amd.knn import build_ivfpq_index_device, synth_rows_device
    from clip_retrieval_amd.service import ArrowMetadataProvider, KnnHotPath, reorder_arrow_metadata

    n, d, k = a.ivf_rows, 1024, 40

    def fill_rows(dst, row0, count, stride):
        synth_rows_device(dst, row0, count, d, 5, kind=1, n_clusters=4096, row_stride=stride)

    ix, _ = build_ivfpq_index_device(fill_rows, n, d, a.nlist, 64, nprobe=16, niter=4, pq_niter=4, seed=0)
    qrows = torch.empty((256, d), dtype=torch.float16, device="cuda")
    synth_rows_device(qrows.data_ptr(), n + 12345, 256, d, 5, kind=1, n_clusters=4096)
    q = qrows.float().cpu().numpy()
    q = np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), dtype=np.float32)
    tmp = tempfile.mkdtemp(prefix="reqserve")
    ids = pa.array(np.arange(n, dtype=np.int64))
    table = pa.table({"url": pc.binary_join_element_wise(pa.scalar("https://example.org/images/"), pc.cast(ids, pa.string()), pa.scalar(".jpg"), pa.scalar("")),
                      "row": ids})
    mdir = os.path.join(tmp, "meta")
    os.makedirs(mdir)
    with pa.OSFile(os.path.join(mdir, "0.arrow"), "wb") as sink, pa.ipc.new_file(sink, table.schema) as w:
        w.write_table(table, max_chunksize=1 << 20)
    del table
    reorder_s = None
    if a.ordered_by_ivf:
        t0 = time.perf_counter()
        mdir2 = os.path.join(tmp, "meta_by_list")
        reorder_arrow_metadata(ix, mdir, mdir2)
        reorder_s = time.perf_counter() - t0
        mdir = mdir2
    provider = ArrowMetadataProvider(mdir)
    res = SimpleNamespace(image_index=ix, text_index=ix, metadata_is_ordered_by_ivf=bool(a.ordered_by_ivf), ivf_old_to_new_mapping=None,
                          safety_model=None, violence_detector=None, aesthetic_embeddings=None)
    hp = KnnHotPath()
    T, R = a.serve_threads, a.requests
    lat = [[] for _ in range(T)]
    rows_seen = [None] * T
    go = threading.Barrier(T + 1)

    def worker(t):
        go.wait()
        for r in range(R):
            t0 = time.perf_counter()
            j = (t * R + r) % 256
            dist, ind = hp.knn_search(q[j:j + 1], "image", k, res, False, False, False)
            meta = hp.map_to_metadata(ind, dist, len(ind), provider, ["url", "row"])
            lat[t].append(time.perf_counter() - t0)
            if r == 0:
                rows_seen[t] = [m["row"] for m in meta]
        go.wait()

    hp.knn_search(q[:1], "image", k, res, False, False, False)  # (first call: kernels loaded, scratch allocated)
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
    for th in threads:
        th.start()
    go.wait()
    t0 = time.perf_counter()
    go.wait()
    wall = time.perf_counter() - t0
    for th in threads:
        th.join()
    # the same records either way: the `row` column carries the original id
    check = all(rows_seen[t] == [int(v) for v in ix.search(q[(t * R) % 256:(t * R) % 256 + 1], k)[1][0] if v >= 0] for t in range(min(T, 4)))
    all_lat = np.sort(np.concatenate([np.asarray(x) for x in lat]))
    print("SERVE " + json.dumps({"rows": n, "nlist": a.nlist, "threads": T, "requests": T * R, "k": k, "ordered_by_ivf": bool(a.ordered_by_ivf),
                                 "requests_per_s": round(T * R / wall, 1), "p50_ms": round(float(all_lat[len(all_lat) // 2]) * 1e3, 3),
                                 "p99_ms": round(float(all_lat[int(len(all_lat) * 0.99)]) * 1e3, 3), "records_are_the_original_rows": bool(check),
                                 "reorder_metadata_s": None if reorder_s is None else round(reorder_s, 2),
                                 "coalesce": ix.coalesce_stats()}), flush=True)


def device_filter(a):
    """--device-filter: request time of knn_search with the post filter on the device against the general path (see the module text)."""
    import threading
    from types import SimpleNamespace

    import numpy as np
    import torch

    from clip_retrieval_amd.knn import Mi355xIndex, build_ivfsq_index_device, synth_rows_device
    from clip_retrieval_amd.service import KnnHotPath, Mi355xSafetyHead
    from clip_retrieval_amd.synth import perturbed_queries

    rng = np.random.default_rng(0)
    if a.filter_index == "flat":
        d = 768
        ix = Mi355xIndex(d)
        rows = int(min(a.rows, (torch.cuda.mem_get_info()[0] - (8 << 30)) // (d * 2)))
        ix.synth_fill(rows, 3)
        q = perturbed_queries(ix.reconstruct_batch(np.sort(rng.choice(rows, 64, replace=False))))
        what = {"index": "flat", "rows": rows, "d": d}
    else:
        d, rows = 1024, a.ivf_rows

        def fill_rows(dst, row0, count, stride):
            synth_rows_device(dst, row0, count, d, 5, kind=1, n_clusters=4096, row_stride=stride)

        ix = build_ivfsq_index_device(fill_rows, rows, d, a.nlist, nprobe=a.nprobe, niter=4, seed=0, threshold_scan=True)[0]
        qrows = torch.empty((64, d), dtype=torch.float16, device="cuda")
        synth_rows_device(qrows.data_ptr(), rows + 12345, 64, d, 5, kind=1, n_clusters=4096)
        q = qrows.float().cpu().numpy()
        q = np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), dtype=np.float32)
        what = {"index": "ivfsq", "rows": rows, "d": d, "nlist": a.nlist, "nprobe": a.nprobe}
    widths, positions = [d, 1024, 2048, 1024, 256, 128, 16, 1], [0, 3, 6, 9, 12, 15, 16]
    sd = {}
    for j, p_ in enumerate(positions):
        sd[f"layers.{p_}.weight"] = (rng.uniform(-1, 1, (widths[j + 1], widths[j])) * np.sqrt(3.0 / widths[j])).astype(np.float32)
        sd[f"layers.{p_}.bias"] = (rng.uniform(-1, 1, widths[j + 1]) * 0.1).astype(np.float32)
    prompts = rng.standard_normal((2, d)).astype(np.float32)
    prompts /= np.linalg.norm(prompts, axis=1, keepdims=True)
    res = SimpleNamespace(image_index=ix, text_index=ix, metadata_is_ordered_by_ivf=False, safety_model=Mi355xSafetyHead(sd, device=0),
                          violence_detector=prompts, aesthetic_embeddings=None)
    hp = {False: KnnHotPath(device_filter=False), True: KnnHotPath(device_filter=True)}
    print(f"index: {what}", flush=True)

    if a.serve_threads:
        T, R, k = a.serve_threads, a.requests, 3000
        for on in (False, True):
            hp[on].knn_search(q[:1], "image", k, res, True, True, True)
            lat = [[] for _ in range(T)]
            go = threading.Barrier(T + 1)

            def worker(t, on=on, lat=lat, go=go):
                go.wait()
                for r in range(R):
                    t0 = time.perf_counter()
                    hp[on].knn_search(q[(t * R + r) % 64:(t * R + r) % 64 + 1], "image", k, res, True, True, True)
                    lat[t].append(time.perf_counter() - t0)
                go.wait()

            threads = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
            for th in threads:
                th.start()
            go.wait()
            t0 = time.perf_counter()
            go.wait()
            wall = time.perf_counter() - t0
            for th in threads:
                th.join()
            all_lat = np.sort(np.concatenate([np.asarray(x) for x in lat]))
            print("FILTER " + json.dumps({**what, "leg": f"--serve-threads {T}", "k": k, "filters": "dedup+violence+safety", "device_filter": on,
                                          "requests": T * R, "requests_per_s": round(T * R / wall, 1),
                                          "p50_ms": round(float(all_lat[len(all_lat) // 2]) * 1e3, 3),
                                          "p99_ms": round(float(all_lat[int(len(all_lat) * 0.99)]) * 1e3, 3)}), flush=True)
        return

    for k in (40, 3000):
        for name, flags in (("dedup", (True, False, False)), ("dedup+violence+safety", (True, True, True))):
            same = True
            for on in (False, True):  # (first calls: kernels loaded, scratch allocated, prompt heads cached)
                hp[on].knn_search(q[:1], "image", k, res, *flags)
            med = {False: [], True: []}
            for rnd in range(a.rounds):
                for on in ((False, True) if rnd % 2 == 0 else (True, False)):
                    ts = []
                    for r in range(a.reps):
                        j = (rnd * a.reps + r) % 64
                        t0 = time.perf_counter()
                        got = hp[on].knn_search(q[j:j + 1], "image", k, res, *flags)
                        ts.append(time.perf_counter() - t0)
                        if r == 0 and on:
                            ref = hp[False].knn_search(q[j:j + 1], "image", k, res, *flags)
                            same = same and [int(i) for i in ref[1]] == [int(i) for i in got[1]]
                    med[on].append(float(np.median(ts)) * 1e3)
            line = {**what, "k": k, "filters": name, "rounds": a.rounds, "reps": a.reps, "same_ids_as_the_general_path": bool(same)}
            for on, key in ((False, "general_path_ms"), (True, "device_filter_ms")):
                m = np.asarray(med[on])
                line[key] = {"median": round(float(np.median(m)), 3), "min": round(float(m.min()), 3), "max": round(float(m.max()), 3)}
            print("FILTER " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-filter", action="store_true", help="measure knn_search with the post filter on the device against the general path")
    ap.add_argument("--filter-index", choices=("flat", "ivfsq"), default="flat", help="with --device-filter: the index served")
    ap.add_argument("--nprobe", type=int, default=64, help="with --device-filter --filter-index ivfsq")
    ap.add_argument("--rounds", type=int, default=5, help="with --device-filter: rounds (both switch positions in each)")
    ap.add_argument("--serve-threads", type=int, default=0, help="measure the serving side alone from this many request threads (see the module text)")
    ap.add_argument("--ordered-by-ivf", action="store_true", help="with --serve-threads: serve with metadata_is_ordered_by_ivf=True")
    ap.add_argument("--ivf-rows", type=int, default=16_777_216)
    ap.add_argument("--nlist", type=int, default=16384)
    ap.add_argument("--requests", type=int, default=200, help="with --serve-threads: requests per thread")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--meta-rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model", default="ViT-L/14")
    a = ap.parse_args()
    if a.ordered_by_ivf and not a.serve_threads:
        ap.error("--ordered-by-ivf needs --serve-threads")
    if a.device_filter:
        device_filter(a)
        return
    if a.serve_threads:
        serve(a)
        return

    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    import torch
    from PIL import Image
    from types import SimpleNamespace

    from clip_retrieval_amd.encoder import load_clip
    from clip_retrieval_amd.knn import Mi355xIndex
    from clip_retrieval_amd.service import ArrowMetadataProvider, KnnHotPath
    from clip_retrieval_amd.synth import perturbed_queries

    tmp = tempfile.mkdtemp(prefix="reqbench")
    synthetic_merges(tmp)
    model, preprocess, tokenizer = load_clip("random:" + a.model, warmup_batch_size=1, clip_cache_path=tmp)
    d = 768
    ix = Mi355xIndex(d)
    free = torch.cuda.mem_get_info()[0]
    rows = int(min(a.rows, (free - (8 << 30)) // (d * 2)))
    ix.synth_fill(rows, 3)
    print(f"index: {rows} x {d} fp16 = {rows * d * 2 / 1e9:.1f} GB resident; metadata table: {a.meta_rows} rows", flush=True)

    # metadata: Arrow IPC file, memory-mapped like the reference's provider
    ids = pa.array(np.arange(a.meta_rows, dtype=np.int64))
    s = pc.cast(ids, pa.string())
    table = pa.table({"url": pc.binary_join_element_wise(pa.scalar("https://example.org/images/"), s, pa.scalar(".jpg"), pa.scalar("")),
                      "caption": pc.binary_join_element_wise(pa.scalar("a synthetic caption for image number "), s, pa.scalar("")),
                      "width": pa.array(np.full(a.meta_rows, 512, dtype=np.int32))})
    mdir = os.path.join(tmp, "meta")
    os.makedirs(mdir)
    with pa.OSFile(os.path.join(mdir, "0.arrow"), "wb") as sink:
        with pa.ipc.new_file(sink, table.schema) as w:
            w.write_table(table, max_chunksize=1 << 20)
    del table
    fast = ArrowMetadataProvider(mdir)
    slow = ReferenceStyleProvider(fast.table)

    res = SimpleNamespace(model=model, tokenizer=tokenizer, preprocess=preprocess, device="cuda:0", image_index=ix, text_index=ix,
                          metadata_is_ordered_by_ivf=False, safety_model=None, violence_detector=None, aesthetic_embeddings=None)
    hp = KnnHotPath()
    rng = np.random.default_rng(0)
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)).save(buf, format="JPEG", quality=90)
    img_b64 = base64.b64encode(buf.getvalue()).decode()
    planted = rng.choice(rows, 64, replace=False)
    qemb = perturbed_queries(ix.reconstruct_batch(np.sort(planted)))

    def timed(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        ts = np.sort(ts)
        return out, float(np.mean(ts)) * 1e3, float(ts[len(ts) // 2]) * 1e3, float(ts[-1]) * 1e3

    stages = {}
    _, m, p50, mx = timed(lambda: hp.compute_query(res, "a photo of the red car on beach at night", None, None, None), a.reps)
    stages["text_query_B1"] = (m, p50, mx)
    _, m, p50, mx = timed(lambda: hp.compute_query(res, None, img_b64, None, None), a.reps)
    stages["image_query_B1 (incl. JPEG decode + preprocess)"] = (m, p50, mx)
    pil = Image.open(io.BytesIO(base64.b64decode(img_b64)))
    px = preprocess(pil).unsqueeze(0)
    _, m, p50, mx = timed(lambda: model.encode_image(px), a.reps)
    stages["image_encode_only_B1"] = (m, p50, mx)
    out = {"rows": rows, "meta_rows": a.meta_rows, "stages_ms": {}, "requests": []}
    for k, dedup in ((40, False), (40, True), (3000, False), (3000, True)):
        j = [0]

        def search():
            j[0] += 1
            return hp.knn_search(qemb[j[0] % 64:j[0] % 64 + 1], "image", k, res, dedup, False, False)

        (dist, ind), m, p50, mx = timed(search, max(3, a.reps // (1 if k <= 64 else 4)))
        stages[f"knn_search k={k}{' +dedup' if dedup else ''}"] = (m, p50, mx)
        ind_m = [np.int64(int(i) % a.meta_rows) for i in ind]  # the metadata table is smaller than the index: fold the ids
        nimg = min(len(ind_m), k)
        _, ms_fast, _, _ = timed(lambda: hp.map_to_metadata(ind_m, dist, nimg, fast, ["url", "caption"]), a.reps)
        _, ms_slow, _, _ = timed(lambda: hp.map_to_metadata(ind_m, dist, nimg, slow, ["url", "caption"]), max(3, a.reps // 4))
        stages[f"map_to_metadata k={k}: batched take"] = (ms_fast, ms_fast, ms_fast)
        stages[f"map_to_metadata k={k}: reference-style per-id slices"] = (ms_slow, ms_slow, ms_slow)
        if not dedup:
            def request():
                q = hp.compute_query(res, "a photo of the red car on beach at night", None, None, None)
                dd, ii = hp.knn_search(q, "image", k, res, True, False, False)
                return hp.map_to_metadata([np.int64(int(i) % a.meta_rows) for i in ii], dd, len(ii), fast, ["url", "caption"])

            _, m, p50, mx = timed(request, max(3, a.reps // (1 if k <= 64 else 4)))
            out["requests"].append({"k": k, "deduplicate": True, "mean_ms": round(m, 3), "p50_ms": round(p50, 3), "max_ms": round(mx, 3)})
            stages[f"WHOLE REQUEST text -> k={k} +dedup -> metadata"] = (m, p50, mx)
    # safety head of the post filter (clip_back.py:315-325; H14 detector stack, h14_nsfw_model.py:16-34) on k result embeddings:
    # GPU (service.Mi355xSafetyHead) vs the reference's torch fp32 module on this box's host cores (random weights: same arithmetic)
    from clip_retrieval_amd.service import Mi355xSafetyHead

    widths, positions = [1024, 1024, 2048, 1024, 256, 128, 16, 1], [0, 3, 6, 9, 12, 15, 16]
    sd, layers = {}, []
    for j, p_ in enumerate(positions):
        lin = torch.nn.Linear(widths[j], widths[j + 1])
        sd[f"layers.{p_}.weight"], sd[f"layers.{p_}.bias"] = lin.weight.data, lin.bias.data
        layers.append(lin)
        if j + 1 < len(positions) and positions[j + 1] != p_ + 1:
            layers += [torch.nn.ReLU(), torch.nn.Dropout(0.2)]
    ref_head = torch.nn.Sequential(*layers).eval()
    head = Mi355xSafetyHead(sd, device=0)
    for k in (40, 3000):
        e = rng.standard_normal((k, 1024)).astype(np.float32)
        _, m, p50, mx = timed(lambda: head.predict(e, batch_size=k), a.reps)
        stages[f"safety head k={k}: GPU (incl. H2D / D2H)"] = (m, p50, mx)

        def ref_predict():
            with torch.no_grad():
                return ref_head(torch.from_numpy(e)).numpy()

        _, m, p50, mx = timed(ref_predict, a.reps)
        stages[f"safety head k={k}: reference torch fp32 on the host"] = (m, p50, mx)
    print(f"{'stage':70s} {'mean ms':>10s} {'p50 ms':>10s} {'max ms':>10s}")
    for name, (m, p50, mx) in stages.items():
        print(f"{name:70s} {m:10.3f} {p50:10.3f} {mx:10.3f}")
        out["stages_ms"][name] = round(m, 3)
    print("REQUEST " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
