"""Growing a built IVF index on one MI355X: for each kind (IVF-Flat, IVF-PQ, IVF-SQ8) build the index over --rows rows of the synthetic
mixture corpus generated on the device, append --append further rows that are already in HBM (Mi355xIndex.ivf_append_device), and report
  * the time of the call split into assign / move (and the idmap / inv pass inside it) / fill (scatter or encode) -- knnx_ivf_grow_stats;
  * the move's bytes per second next to a hipMemcpyAsync device-to-device copy of the same number of bytes in the same run;
  * the whole call next to a full device rebuild over rows + append rows, the only way to get there without these entry points.  The
    IVF-PQ and IVF-SQ8 rebuilds are handed the first build's centroids and quantiser (no training: assignment and encoding only), and
    their list order is compared with the grown index's; the IVF-Flat device builder always trains, so its train_s is shown apart.
Prints one line per step and ONE JSON line at the end.

  python tools/ivf_append_bench.py                              # 16 M x 1024, nlist 16 384, + 1 M rows, all three kinds
  python tools/ivf_append_bench.py --kinds sq --rows 4000000 --d 768 --nlist 4096
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
    ap.add_argument("--append", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=16384)
    ap.add_argument("--M", type=int, default=64)
    ap.add_argument("--clusters", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--kinds", default="flat,pq,sq")
    ap.add_argument("--copy-reps", type=int, default=3)
    a = ap.parse_args()

    import torch

    from clip_retrieval_amd import load_library
    from clip_retrieval_amd._lib import check
    from clip_retrieval_amd.knn import (build_ivf_index_device, build_ivfpq_index_device, build_ivfsq_index_device, synth_rows_device,
                                        _release_cached_device_memory)

    lib = load_library()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    n, m, d = a.rows, a.append, a.d

    def fill_rows(dst, row0, count, stride):
        synth_rows_device(dst, row0, count, d, a.seed, kind=1, n_clusters=a.clusters, row_stride=stride)
        torch.cuda.synchronize()

    def build(kind, rows, like=None):
        """(index, stats, seconds); like: an index whose centroids and quantiser the build is handed (IVF-PQ, IVF-SQ8)."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "flat":
            ix, st = build_ivf_index_device(fill_rows, rows, d, a.nlist, nprobe=16, niter=6, seed=0)
        elif kind == "pq":
            kw = {} if like is None else {"centroids": like.ivf_centroids, "codebooks": like.pq_codebooks()}
            ix, st = build_ivfpq_index_device(fill_rows, rows, d, a.nlist, a.M, nprobe=16, niter=6, pq_niter=8, seed=0, **kw)
        else:
            kw = {} if like is None else {"centroids": like.ivf_centroids, "ranges": like.sq_quantizer()}
            ix, st = build_ivfsq_index_device(fill_rows, rows, d, a.nlist, nprobe=16, niter=6, seed=0, **kw)
        torch.cuda.synchronize()
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

    out = {"rows": n, "append": m, "d": d, "nlist": a.nlist, "M": a.M}
    for kind in [k for k in a.kinds.split(",") if k]:
        ix, st, base_s = build(kind, n)
        print(f"{kind}: built {n} rows in {base_s:.2f} s (train {st['train_s']:.2f}, assign {st['assign_s']:.2f})", flush=True)
        rows = torch.empty((m, d), dtype=torch.float16, device="cuda")
        fill_rows(rows.data_ptr(), n, m, 1)
        ix.search(np.zeros((1, d), np.float32), 10)  # (a served index: its scratch exists and is dropped by the call)
        t0 = time.perf_counter()
        ids = ix.ivf_append_device(rows.data_ptr(), m)
        append_s = time.perf_counter() - t0
        del rows
        assert ix.ntotal == n + m and ids[-1] == n + m - 1
        am, mm, im, fm, mb = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        check(lib, lib.knnx_ivf_grow_stats(ix._h, C.byref(am), C.byref(mm), C.byref(im), C.byref(fm), C.byref(mb)), "knnx")  # pylint: disable=protected-access
        _release_cached_device_memory()
        copy_s = memcpy_seconds(int(mb.value))
        e = {"base_build_s": round(base_s, 2), "append_s": round(append_s, 3), "assign_ms": round(am.value, 2), "move_ms": round(mm.value, 2),
             "move_ids_ms": round(im.value, 2), "fill_ms": round(fm.value, 2), "moved_bytes": int(mb.value),
             "move_TBps_copied": round(mb.value / (mm.value * 1e-3) / 1e12, 3) if mm.value else None,
             "memcpy_ms": round(copy_s * 1e3, 2), "memcpy_TBps_copied": round(mb.value / copy_s / 1e12, 3),
             "move_over_memcpy": round(mm.value * 1e-3 / copy_s, 3) if copy_s else None}
        print(f"{kind}: appended {m} rows in {append_s:.3f} s: assign {am.value:.1f} ms, move {mm.value:.2f} ms, {im.value:.2f} of it idmap / inv "
              f"({e['move_TBps_copied']} TB/s copied), fill {fm.value:.1f} ms; hipMemcpyAsync of the same {mb.value} bytes {copy_s * 1e3:.1f} ms ({e['memcpy_TBps_copied']} TB/s)",
              flush=True)
        grown_order = ix.ivf_new_to_old() if kind != "flat" else None
        like = ix if kind != "flat" else None
        re, rs, rebuild_s = build(kind, n + m, like)
        e.update({"rebuild_s": round(rebuild_s, 2), "rebuild_train_s": round(rs["train_s"], 2), "rebuild_assign_s": round(rs["assign_s"], 2),
                  "rebuild_fill_s": round(rs.get("encode_s", rs.get("scatter_s", 0.0)), 2),
                  "rebuild_over_append": round((rebuild_s - (rs["train_s"] if kind == "flat" else 0.0)) / append_s, 1)})
        if grown_order is not None:
            e["same_list_order_as_rebuild"] = bool(np.array_equal(grown_order, re.ivf_new_to_old()))
        print(f"{kind}: rebuilt {n + m} rows in {rebuild_s:.2f} s (train {rs['train_s']:.2f}, assign {rs['assign_s']:.2f}, "
              f"fill {e['rebuild_fill_s']:.2f}); list order equal: {e.get('same_list_order_as_rebuild')}", flush=True)
        out[kind] = e
        ix.close()
        re.close()
        del grown_order
        _release_cached_device_memory()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
