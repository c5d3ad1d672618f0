"""IVF-PQ benchmark on one MI355X: build (train / assign / encode) over the synthetic mixture corpus generated on the device
(knnx_synth_rows_device kind 1, BASELINE config 5), HBM bytes per row, QPS at B x nprobe, the ADC scan's kernel time against the
byte model, recall@40 against the exact top-40 streamed over the same corpus, and an IVF-Flat A/B in the same process (--flat-ab,
at a size where both fit).  Prints ONE JSON line.

  python tools/ivfpq_bench.py                                   # config 5's shard: 125 M x 1024, nlist 65 536, M = 64
  python tools/ivfpq_bench.py --rows 1000000000 --d 768         # the headline index on one GPU
  python tools/ivfpq_bench.py --rows 16000000 --nlist 16384 --flat-ab
  python tools/ivfpq_bench.py --rows 16000000 --d 768 --nlist 16384 --M 256 --nprobes 16,64
                                                                # PQ256x8 (the two-half ADC scan; yardstick: the same line with --M 128);
                                                                # also prints the partial-sum slab and the sub-groups of a 256-query pass
  python tools/ivfpq_bench.py --opq                             # + the same index behind an OPQ rotation: rotate_s, recall, times
  python tools/ivfpq_bench.py --opq --kind 2                    # ... on the dominant-column corpus (knnx_synth_rows_device kind 2)
  python tools/ivfpq_bench.py --rows 4000000 --d 512 --nlist 4096 --M 256 --opq --opq-dim 768
                                                                # OPQ256_768 on 512-d rows: ONLY the rectangular index (rotation [768, 512]) and
                                                                # its yardstick, the square d = 768 index over the same rows zero-padded, both
                                                                # with a refine store, built and timed alternately in this process
  python tools/ivfpq_bench.py --rows 16000000 --nlist 16384 --nprobes 64 --refine [--k-factor 1,4,8]
                                                                # + the same index with a refine store and IVF-Flat on the same rows, all three
                                                                # resident, timed alternately; recall@40 of each
  python tools/ivfpq_bench.py --rows 16000000 --nlist 16384 --nprobes 64 --refine --large-k 100,3000
                                                                # + one query at nprobe 64 for every k on those three indexes (threshold scan
                                                                # switched on), timed alternately; threshold scans and hits fetched per query
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=65536)
    ap.add_argument("--M", type=int, default=64)
    ap.add_argument("--clusters", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--batches", default="1,32,256")
    ap.add_argument("--nprobes", default="16,64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--recall-queries", type=int, default=64)
    ap.add_argument("--flat-ab", action="store_true")
    ap.add_argument("--opq", action="store_true", help="also build the index behind a trained OPQ rotation and compare: same corpus, queries, process")
    ap.add_argument("--opq-dim", type=int, default=0, help="with --opq: d_out > d.  Builds the index behind a trained rotation [d_out, d] and the "
                    "square d_out index over the zero-padded rows (both with a refine store), reports rotate_s, build seconds, arena bytes "
                    "and B x nprobe 64 timed alternately, and nothing else")
    ap.add_argument("--refine", action="store_true", help="also build the index with a refine store (same centroids and codebooks) and IVF-Flat "
                    "on the same rows; all three stay resident and are timed alternately at nprobe 64, k = 40")
    ap.add_argument("--k-factor", default="1,4,8", help="k_factor values of --refine")
    ap.add_argument("--large-k", default="", help="with --refine: k values above 64 (e.g. 100,3000) timed at B = 1, nprobe 64 on the plain index, "
                    "the refine index (the first --k-factor) and IVF-Flat -- the yardstick -- alternately")
    ap.add_argument("--id-order", action="store_true", help="build the index, time the export of its list-ordered ids (Mi355xIndex.ivf_old_to_new / "
                    "ivf_new_to_old: one pass on the device) against the numpy restatement on this box (np.concatenate of the per-list ids, "
                    "inverse by np.put), print one JSON line and stop")
    ap.add_argument("--kind", type=int, default=1, choices=(1, 2), help="corpus: 1 = the mixture of config 5, 2 = isotropic with three dominant columns")
    a = ap.parse_args()

    import torch

    from clip_retrieval_amd.knn import Mi355xIndex, build_ivf_index_device, build_ivfpq_index_device, synth_rows_device

    n, d = a.rows, a.d

    def fill_rows(dst, row0, count, stride):
        if a.kind == 1:
            synth_rows_device(dst, row0, count, d, a.seed, kind=1, n_clusters=a.clusters, row_stride=stride)
            return
        # kind 2 is generated with stride 1 only; its rows are i.i.d., so a contiguous block is as good a sample as a strided one
        synth_rows_device(dst, row0, count, d, a.seed, kind=2)

    if a.opq_dim:
        if not a.opq:
            ap.error("--opq-dim needs --opq")
        print(json.dumps(rect_ab(a, fill_rows)))
        return

    free0 = torch.cuda.mem_get_info()[0]
    index, st = build_ivfpq_index_device(fill_rows, n, d, a.nlist, a.M, nprobe=16, niter=6, pq_niter=8, seed=0)
    torch.cuda.synchronize()
    if a.id_order:
        print(json.dumps(id_order_ab(a, index, st)))
        return
    used = free0 - torch.cuda.mem_get_info()[0]
    out = {"rows": n, "d": d, "nlist": a.nlist, "M": a.M, "train_s": round(st["train_s"], 2), "assign_s": round(st["assign_s"], 2),
           "encode_s": round(st["encode_s"], 2), "bytes_per_row_model": a.M + 12, "hbm_bytes_index": int(used),
           "hbm_bytes_per_row": round(used / n, 2)}

    # queries: corpus rows (a different seed region) perturbed -- the mixture's own distribution
    rng = np.random.default_rng(1)
    qrows = torch.empty((256, d), dtype=torch.float16, device="cuda")
    synth_rows_device(qrows.data_ptr(), n + 12345, 256, d, a.seed, kind=a.kind, n_clusters=a.clusters if a.kind == 1 else 0)
    q = qrows.float().cpu().numpy()
    q += 0.05 * rng.standard_normal(q.shape).astype(np.float32) / np.sqrt(d)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q = np.ascontiguousarray(q, dtype=np.float32)
    qd = torch.from_numpy(q).cuda()
    Dd = torch.empty((256, 64), dtype=torch.float32, device="cuda")
    Id = torch.empty((256, 64), dtype=torch.int64, device="cuda")

    def timed(ix, B, k=40):
        ix.search_device(qd.data_ptr(), B, k, Dd.data_ptr(), Id.data_ptr())
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ix.search_device(qd.data_ptr(), B, k, Dd.data_ptr(), Id.data_ptr())
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    grid = {}
    for npb in [int(v) for v in a.nprobes.split(",")]:
        index.nprobe = npb
        for B in [int(v) for v in a.batches.split(",")]:
            t = timed(index, B)
            index.profile(True)
            index.search_device(qd.data_ptr(), B, 40, Dd.data_ptr(), Id.data_ptr())
            torch.cuda.synchronize()
            _, scan_ms = index.profile_get()
            index.profile(False)
            code_bytes = B * npb * (n / a.nlist) * a.M  # byte model: every probed list's codes once per query
            grid[f"B{B}_np{npb}"] = {"ms": round(t * 1e3, 3), "qps": round(B / t, 1), "adc_scan_ms": round(scan_ms, 3),
                                     "code_bytes_model": int(code_bytes), "code_TBps_model": round(code_bytes / (scan_ms * 1e-3) / 1e12, 2) if scan_ms else None}
    out["search"] = grid
    if a.M == 256:
        # the two-half ADC scan's partial sums (csrc/knnx_pq_plan.h): slab = the nprobe largest lists, and whether the budget cut a
        # 256-query pass into sub-groups
        budget = int(os.environ.get("KNNX_PQ_PARTIAL_MAX_BYTES") or 0) or 1 << 30
        sizes = np.sort(np.asarray(st["list_sizes"], dtype=np.int64))[::-1]
        out["partial_sums"] = {"budget_bytes": budget}
        for npb in [int(v) for v in a.nprobes.split(",")]:
            slab = int(sizes[:npb].sum())
            g = min(256, max(1, budget // max(slab * 4, 1)))
            out["partial_sums"][f"np{npb}"] = {"slab_rows": slab, "bytes_B256": min(g, 256) * slab * 4, "sub_groups_B256": -(-256 // g)}

    # recall@40 at nprobe 64 against the exact top-40, streamed over the corpus in chunks (flat scans of device-generated rows)
    nr, k = a.recall_queries, 40
    index.nprobe = 64
    _, I_pq = index.search(q[:nr], k)
    chunk = 1 << 23
    buf = torch.empty((min(chunk, n), d), dtype=torch.float16, device="cuda")
    best_D = np.full((nr, k), -np.inf, np.float32)
    best_I = np.full((nr, k), -1, np.int64)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        synth_rows_device(buf.data_ptr(), o, m, d, a.seed, kind=a.kind, n_clusters=a.clusters if a.kind == 1 else 0)
        torch.cuda.synchronize()
        f = Mi355xIndex(d, id_base=o)
        f.attach_device_rows(buf.data_ptr(), m)
        D, I = f.search(q[:nr], k)
        f.close()
        allD, allI = np.concatenate([best_D, D], 1), np.concatenate([best_I, I], 1)
        sel = np.argsort(-allD, axis=1, kind="stable")[:, :k]
        best_D, best_I = np.take_along_axis(allD, sel, 1), np.take_along_axis(allI, sel, 1)
    del buf
    out["recall40_np64"] = round(float(np.mean([len(set(x) & set(y)) / k for x, y in zip(I_pq, best_I)])), 4)

    if a.opq:
        # the same index behind a trained rotation, in the same process; the two are timed alternately (box-to-box spread is ~5 %)
        rot, so = build_ivfpq_index_device(fill_rows, n, d, a.nlist, a.M, nprobe=64, niter=6, pq_niter=8, seed=0, opq=True)
        torch.cuda.synchronize()
        index.nprobe = rot.nprobe = 64
        _, I_rot = rot.search(q[:nr], k)
        cmp_ = {"opq_s": round(so["opq_s"], 2), "train_s": round(so["train_s"], 2), "assign_s": round(so["assign_s"], 2),
                "rotate_s": round(so["rotate_s"], 2), "encode_s": round(so["encode_s"], 2),
                "recall40_np64": round(float(np.mean([len(set(x) & set(y)) / k for x, y in zip(I_rot, best_I)])), 4),
                "recall40_np64_plain": out["recall40_np64"]}
        for B in [int(v) for v in a.batches.split(",")]:
            tp, tr = [], []
            for _ in range(3):
                tp.append(timed(index, B))
                tr.append(timed(rot, B))
            cmp_[f"B{B}_np64_ms_plain"] = round(float(np.median(tp)) * 1e3, 4)
            cmp_[f"B{B}_np64_ms"] = round(float(np.median(tr)) * 1e3, 4)
        out["opq"] = cmp_
        rot.close()

    if a.refine:
        # the same centroids and codebooks (so the candidates are the plain index's), the fp16 rows next to the codes; IVF-Flat with the
        # same k-means seed on the same rows.  One process, the indexes timed alternately, three rounds, the median of the rounds' medians.
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        ref, sr = build_ivfpq_index_device(fill_rows, n, d, a.nlist, a.M, nprobe=64, seed=0, centroids=index.ivf_centroids,
                                           codebooks=index.pq_codebooks(), refine=True)
        torch.cuda.synchronize()
        used_ref = free1 - torch.cuda.mem_get_info()[0]
        flat, sf = build_ivf_index_device(fill_rows, n, d, a.nlist, nprobe=64, seed=0)
        index.nprobe = ref.nprobe = flat.nprobe = 64
        kfs = [int(v) for v in a.k_factor.split(",")]

        def rec(I):
            return round(float(np.mean([len(set(x) & set(y)) / k for x, y in zip(I, best_I)])), 4)

        r = {"assign_s": round(sr["assign_s"], 2), "encode_s": round(sr["encode_s"], 2), "code_arena_bytes": sr["code_arena_bytes"],
             "row_arena_bytes": sr["row_arena_bytes"], "hbm_bytes_index": int(used_ref), "hbm_bytes_plain": int(used),
             "flat_build_s": round(sum(v for kk, v in sf.items() if kk.endswith("_s")), 2) if isinstance(sf, dict) else None,
             "recall40_plain": rec(index.search(q[:nr], k)[1]), "recall40_ivf_flat": rec(flat.search(q[:nr], k)[1])}
        for kf in kfs:
            ref.k_factor = kf
            r[f"recall40_kf{kf}"] = rec(ref.search(q[:nr], k)[1])
        for B in [int(v) for v in a.batches.split(",")]:
            ts = {"plain": [], "ivf_flat": [], **{f"kf{kf}": [] for kf in kfs}}
            for _ in range(3):
                ts["plain"].append(timed(index, B))
                for kf in kfs:
                    ref.k_factor = kf
                    ts[f"kf{kf}"].append(timed(ref, B))
                ts["ivf_flat"].append(timed(flat, B))
            for name, v in ts.items():
                r[f"B{B}_np64_ms_{name}"] = round(float(np.median(v)) * 1e3, 4)
        out["refine"] = r
        if a.large_k:
            # k > 64 through the threshold scan (Mi355xIndex.pq_threshold_scan): host-buffer searches of ONE query, the three indexes
            # alternately, three rounds of --reps, the median of the rounds' medians.  IVF-Flat's time for the same k is the yardstick.
            index.pq_threshold_scan = ref.pq_threshold_scan = True
            ref.k_factor = kfs[0]

            def timed_host(ix, kk):
                ix.search(q[:1], kk)
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    ix.search(q[:1], kk)
                    ts.append(time.perf_counter() - t0)
                return float(np.median(ts))

            lk = {"k_factor": kfs[0]}
            for kk in [64] + [int(v) for v in a.large_k.split(",")]:
                ts = {"plain": [], "refine": [], "ivf_flat": []}
                s0, s1 = index.pq_threshold_stats(), ref.pq_threshold_stats()
                for _ in range(3):
                    ts["plain"].append(timed_host(index, kk))
                    if kk > 64 or kk * kfs[0] <= 512:
                        ts["refine"].append(timed_host(ref, kk))
                    ts["ivf_flat"].append(timed_host(flat, kk))
                e = {f"ms_{name}": round(float(np.median(v)) * 1e3, 4) for name, v in ts.items() if v}
                for name, ix, before in (("plain", index, s0), ("refine", ref, s1)):
                    nq, _, qs, hits = (x - y for x, y in zip(ix.pq_threshold_stats(), before))
                    if nq:
                        e[f"scans_per_query_{name}"] = round(qs / nq, 2)
                        e[f"hits_per_query_{name}"] = round(hits / nq, 1)
                lk[f"k{kk}"] = e
            out["large_k"] = lk
        ref.close()
        flat.close()

    if a.flat_ab:
        index.close()
        torch.cuda.empty_cache()
        flat, _ = build_ivf_index_device(fill_rows, n, d, a.nlist, nprobe=64, seed=0)  # same k-means seed: the same coarse centroids
        flat.nprobe = 64
        _, I_f = flat.search(q[:nr], k)
        ab = {"recall40_np64": round(float(np.mean([len(set(x) & set(y)) / k for x, y in zip(I_f, best_I)])), 4)}
        for B in (1, 256):
            t = timed(flat, B)
            ab[f"B{B}_np64_ms"] = round(t * 1e3, 3)
        out["ivf_flat_ab"] = ab
        flat.close()
    else:
        index.close()
    print(json.dumps(out))


def id_order_ab(a, index, st):
    """The export of the list-ordered ids against the numpy restatement of ivf_metadata_ordering.py:46-64 (the reference's own loop needs
    faiss): per-list id arrays -> np.concatenate, inverse by np.put.  The per-list arrays are views of the exported new_to_old, cut at
    the list sizes, so the yardstick starts from what il.get_ids(l) would hand it."""
    def best(fn, reps):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
        return r, float(np.min(ts)), float(np.median(ts))

    index.ivf_old_to_new()  # (first call: dense0 is built, the runtime has loaded the kernels)
    o2n, o2n_min, o2n_med = best(index.ivf_old_to_new, a.reps)
    n2o, n2o_min, n2o_med = best(index.ivf_new_to_old, a.reps)
    sizes = np.asarray(st["list_sizes"], dtype=np.int64)
    per_list = np.split(n2o, np.cumsum(sizes)[:-1])

    def restated():
        flat = np.concatenate(per_list)
        d_ = np.ones((flat.shape[0],), "int64")
        d_.put(flat, np.arange(flat.shape[0], dtype=np.int64))
        return flat, d_

    (flat, inv), np_min, np_med = best(restated, a.reps)
    ids = np.random.default_rng(0).integers(0, a.rows, 40).astype(np.int64)
    index.map_ids(ids)
    _, map_min, map_med = best(lambda: index.map_ids(ids), 200)
    return {"rows": a.rows, "d": a.d, "nlist": a.nlist, "M": a.M, "equal_to_numpy": bool(np.array_equal(flat, n2o) and np.array_equal(inv, o2n)),
            "empty_lists": int((sizes == 0).sum()), "largest_list": int(sizes.max()),
            "old_to_new_s": {"min": round(o2n_min, 4), "median": round(o2n_med, 4)},
            "new_to_old_s": {"min": round(n2o_min, 4), "median": round(n2o_med, 4)},
            "numpy_concatenate_put_s": {"min": round(np_min, 4), "median": round(np_med, 4)},
            "map_ids_40_us": {"min": round(map_min * 1e6, 1), "median": round(map_med * 1e6, 1)}}


def rect_ab(a, fill_rows):
    """--opq --opq-dim N: the index with two widths (rows d, quantiser d_out = N) against the route it replaces -- every row and query
    zero-padded to N in front of a square N rotation.  Same rows, same seeds (the two rotations are trained by the same recipe on the
    same padded sample), both with a refine store; searches alternate between the two, three rounds, the median of the rounds' medians."""
    import torch

    from clip_retrieval_amd.knn import build_ivfpq_index_device, opq_embedding, rotate_rows_device, synth_rows_device

    n, d, dq, k = a.rows, a.d, a.opq_dim, 40
    E = opq_embedding(d, dq)

    def fill_padded(dst, row0, count, stride):  # the same rows, N wide: generated d wide, then scattered into zeros (exact)
        tmp = torch.empty((count, d), dtype=torch.float16, device="cuda")
        fill_rows(tmp.data_ptr(), row0, count, stride)
        torch.cuda.synchronize()
        rotate_rows_device(E, tmp.data_ptr(), count, dst, 0)

    out = {"rows": n, "d": d, "d_out": dq, "nlist": a.nlist, "M": a.M}
    built = {}
    for name, fill, width, kw in (("rect", fill_rows, d, {"opq_dim": dq}), ("padded_square", fill_padded, dq, {})):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix, st = build_ivfpq_index_device(fill, n, width, a.nlist, a.M, nprobe=64, niter=6, pq_niter=8, seed=0, opq=True, refine=True, **kw)
        torch.cuda.synchronize()
        built[name] = ix
        out[name] = {"build_s": round(time.perf_counter() - t0, 2), "opq_s": round(st["opq_s"], 2), "train_s": round(st["train_s"], 2),
                     "assign_s": round(st["assign_s"], 2), "rotate_s": round(st["rotate_s"], 3), "encode_s": round(st["encode_s"], 2),
                     "code_arena_bytes": st["code_arena_bytes"], "row_arena_bytes": st["row_arena_bytes"]}
    qrows = torch.empty((256, d), dtype=torch.float16, device="cuda")
    synth_rows_device(qrows.data_ptr(), n + 12345, 256, d, a.seed, kind=a.kind, n_clusters=a.clusters if a.kind == 1 else 0)
    q = qrows.float().cpu().numpy()
    q += 0.05 * np.random.default_rng(1).standard_normal(q.shape).astype(np.float32) / np.sqrt(d)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    qs = {"rect": torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).cuda(),
          "padded_square": torch.from_numpy(np.ascontiguousarray(np.pad(q, ((0, 0), (0, dq - d))), dtype=np.float32)).cuda()}
    Dd = torch.empty((256, 64), dtype=torch.float32, device="cuda")
    Id = torch.empty((256, 64), dtype=torch.int64, device="cuda")

    def timed(name, B):
        ix, qd = built[name], qs[name]
        ix.search_device(qd.data_ptr(), B, k, Dd.data_ptr(), Id.data_ptr())
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ix.search_device(qd.data_ptr(), B, k, Dd.data_ptr(), Id.data_ptr())
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    ids = {}
    for name, ix in built.items():
        ix.nprobe = 64
        ids[name] = ix.search(qs[name].cpu().numpy(), k)[1]
    out["same_ids_share"] = round(float((ids["rect"] == ids["padded_square"]).mean()), 4)
    for B in [int(v) for v in a.batches.split(",")]:
        ts = {name: [] for name in built}
        for _ in range(3):
            for name in built:
                ts[name].append(timed(name, B))
        for name, v in ts.items():
            out[name][f"B{B}_np64_ms"] = round(float(np.median(v)) * 1e3, 4)
    for ix in built.values():
        ix.close()
    return out


if __name__ == "__main__":
    main()
