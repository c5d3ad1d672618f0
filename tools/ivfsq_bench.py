"""IVF-SQ8 benchmark on one MI355X: build (train / assign / encode) over the synthetic mixture corpus generated on the device
(knnx_synth_rows_device kind 1, BASELINE config 5), HBM bytes against the d + 12 / 2 d + 12 rule, and -- against an IVF-Flat index
built in the same run from the same rows with the same k-means seed (the same centroids and lists), both resident, timed alternately --
batch time and QPS at B x nprobe, the list scan's kernel time and the bytes it walked, and recall@40 of both against the exact top-40
streamed over the same corpus.  Prints ONE JSON line.

  python tools/ivfsq_bench.py                                     # 16 M x 1024, nlist 16 384, nprobe 16 / 64 / 256, B = 1 / 32 / 256
  python tools/ivfsq_bench.py --rows 4000000 --d 768 --nlist 4096
  python tools/ivfsq_bench.py --nprobes 64 --large-k 100,3000      # and k > 64 through the threshold scan, against IVF-Flat's large-k path

--large-k K1,K2: the IVF-SQ8 index is built with its threshold scan switched on (Mi355xIndex.sq_threshold_scan; the k <= 64 paths do not
depend on it); at nprobe 64, for k = 64 and every listed k, one query and a 32-query batch through Mi355xIndex.search (host buffers) on
both indexes alternately, --reps repeats, the median; with the threshold scans per query and the hits fetched per query from
sq_threshold_stats().
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
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=16384)
    ap.add_argument("--clusters", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--batches", default="1,32,256")
    ap.add_argument("--nprobes", default="16,64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--recall-queries", type=int, default=64)
    ap.add_argument("--large-k", default="", help="comma-separated k > 64: time them at nprobe 64 against IVF-Flat (see the module text)")
    a = ap.parse_args()

    import torch

    from clip_retrieval_amd.knn import Mi355xIndex, build_ivf_index_device, build_ivfsq_index_device, synth_rows_device

    n, d, k = a.rows, a.d, 40

    def fill_rows(dst, row0, count, stride):
        synth_rows_device(dst, row0, count, d, a.seed, kind=1, n_clusters=a.clusters, row_stride=stride)

    def built(fn):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter()
        ix, st = fn()
        torch.cuda.synchronize()
        return ix, st, time.perf_counter() - t0, free0 - torch.cuda.mem_get_info()[0]

    large_ks = [int(v) for v in a.large_k.split(",") if v]
    sq, ss, sq_s, sq_used = built(lambda: build_ivfsq_index_device(fill_rows, n, d, a.nlist, nprobe=16, niter=6, seed=0,
                                                                   threshold_scan=bool(large_ks)))
    flat, sf, flat_s, flat_used = built(lambda: build_ivf_index_device(fill_rows, n, d, a.nlist, nprobe=16, niter=6, seed=0))
    padded = int(((np.asarray(ss["list_sizes"]) + 31) // 32 * 32).sum())
    out = {"rows": n, "d": d, "nlist": a.nlist, "padded_rows": padded,
           "same_lists_as_ivf_flat": bool(np.array_equal(ss["list_sizes"], sf["list_sizes"])),
           "sq8": {"build_s": round(sq_s, 2), "train_s": round(ss["train_s"], 2), "assign_s": round(ss["assign_s"], 2),
                   "encode_s": round(ss["encode_s"], 2), "hbm_bytes": int(sq_used), "hbm_bytes_model": padded * (d + 12)},
           "ivf_flat": {"build_s": round(flat_s, 2), "train_s": round(sf["train_s"], 2), "assign_s": round(sf["assign_s"], 2),
                        "scatter_s": round(sf["scatter_s"], 2), "hbm_bytes": int(flat_used), "hbm_bytes_model": padded * (2 * d + 12)}}

    # queries: corpus rows of a region behind the index, perturbed -- the mixture's own distribution
    rng = np.random.default_rng(1)
    qrows = torch.empty((256, d), dtype=torch.float16, device="cuda")
    synth_rows_device(qrows.data_ptr(), n + 12345, 256, d, a.seed, kind=1, n_clusters=a.clusters)
    q = qrows.float().cpu().numpy()
    q += 0.05 * rng.standard_normal(q.shape).astype(np.float32) / np.sqrt(d)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q = np.ascontiguousarray(q, dtype=np.float32)
    qd = torch.from_numpy(q).cuda()
    Dd = torch.empty((256, 64), dtype=torch.float32, device="cuda")
    Id = torch.empty((256, 64), dtype=torch.int64, device="cuda")

    def timed(ix, B):
        ix.search_device(qd.data_ptr(), B, k, Dd.data_ptr(), Id.data_ptr())
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ix.search_device(qd.data_ptr(), B, k, Dd.data_ptr(), Id.data_ptr())
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    def scan(ix, B):  # (kernel ms of the list scan, tiles it walked)
        ix.profile(True)
        ix.search_device(qd.data_ptr(), B, k, Dd.data_ptr(), Id.data_ptr())
        torch.cuda.synchronize()
        _, ms = ix.profile_get()
        ix.profile(False)
        return ms, ix.last_scan_tiles()

    # the exact top-40, streamed over the corpus in chunks (flat scans of device-generated rows)
    nr = a.recall_queries
    chunk = 1 << 22
    buf = torch.empty((min(chunk, n), d), dtype=torch.float16, device="cuda")
    best_D = np.full((nr, k), -np.inf, np.float32)
    best_I = np.full((nr, k), -1, np.int64)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        synth_rows_device(buf.data_ptr(), o, m, d, a.seed, kind=1, n_clusters=a.clusters)
        torch.cuda.synchronize()
        f = Mi355xIndex(d, id_base=o)
        f.attach_device_rows(buf.data_ptr(), m)
        D, I = f.search(q[:nr], k)
        f.close()
        allD, allI = np.concatenate([best_D, D], 1), np.concatenate([best_I, I], 1)
        sel = np.argsort(-allD, axis=1, kind="stable")[:, :k]
        best_D, best_I = np.take_along_axis(allD, sel, 1), np.take_along_axis(allI, sel, 1)
    del buf

    def recall(I, ref):
        return round(float(np.mean([len(set(x) & set(y)) / k for x, y in zip(I, ref)])), 4)

    grid = {}
    for npb in [int(v) for v in a.nprobes.split(",")]:
        sq.nprobe = flat.nprobe = npb
        I_sq, I_fl = sq.search(q[:nr], k)[1], flat.search(q[:nr], k)[1]
        e = {"recall40_sq8": recall(I_sq, best_I), "recall40_ivf_flat": recall(I_fl, best_I), "overlap40_sq8_vs_ivf_flat": recall(I_sq, I_fl)}
        for B in [int(v) for v in a.batches.split(",")]:
            ts, tf = [], []
            for _ in range(3):  # the two indexes alternately, three rounds, the median of the rounds' medians
                ts.append(timed(sq, B))
                tf.append(timed(flat, B))
            t_sq, t_fl = float(np.median(ts)), float(np.median(tf))
            ms_sq, tiles_sq = scan(sq, B)
            ms_fl, tiles_fl = scan(flat, B)
            e[f"B{B}"] = {"ms_sq8": round(t_sq * 1e3, 3), "ms_ivf_flat": round(t_fl * 1e3, 3), "qps_sq8": round(B / t_sq, 1),
                          "qps_ivf_flat": round(B / t_fl, 1), "speedup": round(t_fl / t_sq, 3),
                          "scan_ms_sq8": round(ms_sq, 3), "scan_ms_ivf_flat": round(ms_fl, 3), "scan_tiles_sq8": tiles_sq, "scan_tiles_ivf_flat": tiles_fl,
                          "scan_TBps_sq8": round(tiles_sq * 32 * d / (ms_sq * 1e-3) / 1e12, 2) if ms_sq else None,
                          "scan_TBps_ivf_flat": round(tiles_fl * 32 * d * 2 / (ms_fl * 1e-3) / 1e12, 2) if ms_fl else None}
        grid[f"np{npb}"] = e
    out["search"] = grid

    if large_ks:
        sq.nprobe = flat.nprobe = 64
        lk = {"nprobe": 64, "reps": a.reps}
        for kk in [64] + large_ks:
            e = {}
            for B in (1, 32):
                qq = q[:B]
                sq.search(qq, kk)  # warm-up: pools, pinned staging
                flat.search(qq, kk)
                s0 = sq.sq_threshold_stats()
                ts, tf = [], []
                for _ in range(a.reps):  # the two indexes alternately
                    t0 = time.perf_counter()
                    sq.search(qq, kk)
                    ts.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    flat.search(qq, kk)
                    tf.append(time.perf_counter() - t0)
                s1 = sq.sq_threshold_stats()
                t_sq, t_fl = float(np.median(ts)), float(np.median(tf))
                served = max(1, s1[0] - s0[0])
                e[f"B{B}"] = {"ms_sq8": round(t_sq * 1e3, 3), "ms_ivf_flat": round(t_fl * 1e3, 3), "speedup": round(t_fl / t_sq, 3),
                              "threshold_launches": s1[1] - s0[1],
                              "threshold_scans_per_query": round((s1[2] - s0[2]) / served, 2) if kk > 64 else 0,
                              "hits_fetched_per_query": round((s1[3] - s0[3]) / served, 1) if kk > 64 else 0}
            lk[f"k{kk}"] = e
        for kk in large_ks:
            for B in (1, 32):
                lk[f"k{kk}"][f"B{B}"]["ms_sq8_over_k64"] = round(lk[f"k{kk}"][f"B{B}"]["ms_sq8"] / lk["k64"][f"B{B}"]["ms_sq8"], 2)
        out["large_k"] = lk
    sq.close()
    flat.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
