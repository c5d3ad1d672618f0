"""Shrinking a built IVF index on one MI355X: for each kind (IVF-Flat, IVF-PQ, IVF-SQ8) build the index over --rows rows of the synthetic
mixture corpus generated on the device, remove --remove ids (Mi355xIndex.ivf_remove) in two cases -- uniformly random ids, and the ids
of whole lists (the first lists of the arena, up to the first list boundary at or past --remove rows) -- and report
  * the time of the call split into mark / plan / move / ids -- knnx_ivf_remove_stats;
  * the move's bytes per second next to a hipMemcpyAsync device-to-device copy of the surviving bytes in the same run;
  * the whole call next to a full device rebuild over the surviving rows, the only way to get there without this entry point.  The
    IVF-PQ and IVF-SQ8 rebuilds are handed the first build's centroids and quantiser (no training: assignment and encoding only), and
    their list order is compared with the shrunken index's; the IVF-Flat device builder always trains, so its train_s is taken out.
    The surviving rows are produced for the rebuild by generating the span of source rows a chunk covers and gathering the survivors;
    the time spent producing rows (rows_s) is shown and taken out of the ratio as well, so the ratio counts assignment and fill only.
Prints one line per step and ONE JSON line at the end.

  python tools/ivf_remove_bench.py                              # 16 M x 1024, nlist 16 384, - 1 M rows, all three kinds
  python tools/ivf_remove_bench.py --kinds sq --rows 4000000 --d 768 --nlist 4096
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--remove", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=16384)
    ap.add_argument("--M", type=int, default=64)
    ap.add_argument("--clusters", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--kinds", default="flat,pq,sq")
    ap.add_argument("--cases", default="uniform,lists")
    ap.add_argument("--copy-reps", type=int, default=3)
    a = ap.parse_args()

    import torch

    from clip_retrieval_amd import load_library
    from clip_retrieval_amd.knn import (build_ivf_index_device, build_ivfpq_index_device, build_ivfsq_index_device, synth_rows_device,
                                        _release_cached_device_memory)

    load_library()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    n, m, d = a.rows, a.remove, a.d
    held = []  # (device pointer, tensor) of the builders' scratch, so that a chunk can be written through torch

    def alloc(nbytes):
        t = torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")
        held.append((t.data_ptr(), t))
        return t.data_ptr(), t

    def synth(dst, row0, count, stride):
        synth_rows_device(dst, row0, count, d, a.seed, kind=1, n_clusters=a.clusters, row_stride=stride)

    def fill_rows(dst, row0, count, stride):
        synth(dst, row0, count, stride)
        torch.cuda.synchronize()

    spent = [0.0]

    def survivors(kept_dev):
        """fill_rows over the surviving rows: row i of the rebuild is source row kept[i]."""
        def fill(dst, row0, count, stride):
            t0 = time.perf_counter()
            if stride != 1:  # (a training sample: source rows of the same stride, from the first survivor of the range on)
                synth(dst, int(kept_dev[row0]), count, stride)
            else:
                idx = kept_dev[row0:row0 + count]
                lo, hi = int(idx[0]), int(idx[-1])
                span = torch.empty((hi - lo + 1, d), dtype=torch.float16, device="cuda")
                synth(span.data_ptr(), lo, hi - lo + 1, 1)
                torch.cuda.synchronize()
                base, t = next((p, t) for p, t in held if p <= dst < p + t.numel())
                out = t[dst - base:dst - base + count * d * 2].view(torch.float16).view(count, d)
                torch.index_select(span, 0, idx - lo, out=out)
            torch.cuda.synchronize()
            spent[0] += time.perf_counter() - t0
        return fill

    def build(kind, fill, rows, like=None):
        """(index, stats, seconds); like: an index whose centroids and quantiser the build is handed (IVF-PQ, IVF-SQ8)."""
        del held[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "flat":
            ix, st = build_ivf_index_device(fill, rows, d, a.nlist, nprobe=16, niter=6, seed=0, alloc=alloc)
        elif kind == "pq":
            kw = {} if like is None else {"centroids": like.ivf_centroids, "codebooks": like.pq_codebooks()}
            ix, st = build_ivfpq_index_device(fill, rows, d, a.nlist, a.M, nprobe=16, niter=6, pq_niter=8, seed=0, alloc=alloc, **kw)
        else:
            kw = {} if like is None else {"centroids": like.ivf_centroids, "ranges": like.sq_quantizer()}
            ix, st = build_ivfsq_index_device(fill, rows, d, a.nlist, nprobe=16, niter=6, seed=0, alloc=alloc, **kw)
        torch.cuda.synchronize()
        del held[:]
        return ix, st, time.perf_counter() - t0

    def memcpy_seconds(nbytes):
        """hipMemcpyAsync device to device of nbytes, the median of --copy-reps after one warm-up."""
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        src.zero_()
        ts = []
        for _ in range(a.copy_reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nbytes, 3, None) == 0
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        del src, dst
        _release_cached_device_memory()
        return float(np.median(ts[1:]))

    out = {"rows": n, "remove": m, "d": d, "nlist": a.nlist, "M": a.M}
    rng = np.random.default_rng(a.seed)
    for kind in [k for k in a.kinds.split(",") if k]:
        for case in [c for c in a.cases.split(",") if c]:
            ix, st, base_s = build(kind, fill_rows, n)
            print(f"{kind} / {case}: built {n} rows in {base_s:.2f} s (train {st['train_s']:.2f}, assign {st['assign_s']:.2f})", flush=True)
            ix.search(np.zeros((1, d), np.float32), 10)  # (a served index: its scratch exists and is dropped by the call)
            if case == "uniform":
                ids = rng.choice(n, size=m, replace=False).astype(np.int64)
            else:  # whole lists: inside a list the ids ascend, so a descent of the list-ordered ids is a list boundary
                order = ix.ivf_new_to_old()
                cuts = np.flatnonzero(np.diff(order) < 0) + 1
                ids = np.ascontiguousarray(order[:int(cuts[min(np.searchsorted(cuts, m), len(cuts) - 1)])])
                del order, cuts
            t0 = time.perf_counter()
            kept = ix.ivf_remove(ids)
            remove_s = time.perf_counter() - t0
            assert ix.ntotal == n - len(ids) == len(kept)
            s = ix.ivf_remove_stats()
            device_ms = s["mark_ms"] + s["plan_ms"] + s["move_ms"] + s["ids_ms"]
            _release_cached_device_memory()
            copy_s = memcpy_seconds(int(s["moved_bytes"]))
            e = {"base_build_s": round(base_s, 2), "removed": int(len(ids)), "remove_s": round(remove_s, 4), "device_ms": round(device_ms, 2),
                 "mark_ms": round(s["mark_ms"], 2), "plan_ms": round(s["plan_ms"], 2), "move_ms": round(s["move_ms"], 2),
                 "ids_ms": round(s["ids_ms"], 2), "moved_bytes": int(s["moved_bytes"]),
                 "move_TBps_copied": round(s["moved_bytes"] / (s["move_ms"] * 1e-3) / 1e12, 3) if s["move_ms"] else None,
                 "memcpy_ms": round(copy_s * 1e3, 2), "memcpy_TBps_copied": round(s["moved_bytes"] / copy_s / 1e12, 3),
                 "move_over_memcpy": round(s["move_ms"] * 1e-3 / copy_s, 3) if copy_s else None}
            print(f"{kind} / {case}: removed {len(ids)} rows in {remove_s:.4f} s (numpy bookkeeping of kept included): mark {s['mark_ms']:.2f} ms, "
                  f"plan {s['plan_ms']:.2f} ms, move {s['move_ms']:.2f} ms ({e['move_TBps_copied']} TB/s copied), ids {s['ids_ms']:.2f} ms; "
                  f"hipMemcpyAsync of the same {s['moved_bytes']} bytes {copy_s * 1e3:.2f} ms ({e['memcpy_TBps_copied']} TB/s)", flush=True)
            shrunk_order = ix.ivf_new_to_old() if kind != "flat" else None
            like = ix if kind != "flat" else None
            spent[0] = 0.0
            kept_dev = torch.from_numpy(kept).cuda()
            re, rs, rebuild_s = build(kind, survivors(kept_dev), len(kept), like)
            work_s = rebuild_s - spent[0] - (rs["train_s"] if kind == "flat" else 0.0)
            e.update({"rebuild_s": round(rebuild_s, 2), "rebuild_rows_s": round(spent[0], 2), "rebuild_train_s": round(rs["train_s"], 2),
                      "rebuild_assign_s": round(rs["assign_s"], 2), "rebuild_fill_s": round(rs.get("encode_s", rs.get("scatter_s", 0.0)), 2),
                      "rebuild_work_s": round(work_s, 3), "rebuild_over_remove": round(work_s / remove_s, 1)})
            if shrunk_order is not None:
                e["same_list_order_as_rebuild"] = bool(np.array_equal(shrunk_order, re.ivf_new_to_old()))
            print(f"{kind} / {case}: rebuilt {len(kept)} rows in {rebuild_s:.2f} s ({spent[0]:.2f} of it producing the rows, train {rs['train_s']:.2f}, "
                  f"assign {rs['assign_s']:.2f}, fill {e['rebuild_fill_s']:.2f}): {e['rebuild_over_remove']} x the removal without rows and "
                  f"training; list order equal: {e.get('same_list_order_as_rebuild')}", flush=True)
            out[f"{kind}_{case}"] = e
            ix.close()
            re.close()
            del shrunk_order, kept, kept_dev, ids
            _release_cached_device_memory()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
