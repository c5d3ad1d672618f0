#!/usr/bin/env python3
"""knn_d1280_batch.py [--rows 4194304] [--rounds 5] [--reps 5] [--batches 1,32,64,128,256] [--out FILE] -- what do the one-pass batch
scans buy a flat 1280-wide index?

Unit rows that torch generates in HBM (2^22 x 1280 fp16 = 10.7 GB by default) and THREE handles that borrow them (attach_device_rows),
each created under its own environment:
  exact32  KNNX_RQ=0 KNNX_I8=0   the exact 32-query scan for every group of 32 (what this width did before): the YARDSTICK
  rq_fp16  KNNX_I8=0             the fp16 register-stationary pass (knn_rq16_scan_kernel, 128 queries per pass) for batches above 64
  int8     (nothing set)         the int8 first stage (knn_rq8_scan_kernel<40, ...>) for every batch
One process; after a warm-up of every shape, every round times top-40 searches of every batch size on the three handles in
turn (--batches; host clock around a call that returns host arrays, i.e. ends in a device synchronise; merge and result copy included).  A
round's figure is the median of its repetitions; the report is the median of the round medians with min .. max, the bytes of fp16
rows per second that time corresponds to (the int8 stage reads half of them: its figure is an equivalent rate), the failed proofs of
the timed calls and whether the three forms returned identical ids.  "beats_yardstick": the form's median is below the yardstick's by
more than the yardstick's own min .. max spread in this run -- the rule by which a form is the default at a batch size."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from clip_retrieval_amd.knn import Mi355xIndex  # noqa: E402  pylint: disable=wrong-import-position

D = 1280
FORMS = {"exact32": {"KNNX_RQ": "0", "KNNX_I8": "0"}, "rq_fp16": {"KNNX_I8": "0"}, "int8": {}}


def unit_rows(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((n, D), dtype=torch.float16, device="cuda")
    for o in range(0, n, 1 << 18):
        r = torch.randn((min(1 << 18, n - o), D), generator=g, device="cuda")
        x[o:o + len(r)] = (r / r.norm(dim=1, keepdim=True)).half()
    torch.cuda.synchronize()
    return x


def handle(env, x, n):
    old = {k: os.environ.pop(k, None) for k in ("KNNX_RQ", "KNNX_I8")}
    os.environ.update(env)
    try:
        ix = Mi355xIndex(D, coalesce=False)  # the environment is read when the handle is created
    finally:
        for k in ("KNNX_RQ", "KNNX_I8"):
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    ix.attach_device_rows(x.data_ptr(), n)
    return ix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,32,64,128,256")
    ap.add_argument("--out", default="profiles/knn_d1280_batch.json")
    a = ap.parse_args()
    BATCHES = tuple(int(b) for b in a.batches.split(","))
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    n = a.rows
    x = unit_rows(n, 1280)
    src = np.arange(256) * (n // 256) + 7
    q = x[torch.from_numpy(src).cuda()].float().cpu().numpy()
    q += 0.02 * np.random.default_rng(5).standard_normal(q.shape).astype(np.float32)
    ixs = {name: handle(env, x, n) for name, env in FORMS.items()}
    same, swaps, dmax = True, 0, 0.0
    for B in BATCHES:  # warm-up of every shape (the int8 copy is built here), and the answers of the three forms side by side
        res = {name: ix.search(q[:B], 40) for name, ix in ixs.items()}
        ids = {name: r[1] for name, r in res.items()}
        assert (ids["exact32"][:, 0] == src[:B]).all(), (B, ids["exact32"][:, 0])
        same = same and all(np.array_equal(ids["exact32"], v) for v in ids.values())
        # (the exact scan sums hi / lo MFMA products, the proof-based passes re-score with an fp32 FMA chain: neighbours whose scores
        # differ in the last bit may swap places, so the positions that differ and the largest score difference are reported too)
        swaps += sum(int((ids["exact32"] != v).sum()) for v in ids.values())
        dmax = max(dmax, max(float(np.abs(res["exact32"][0] - r[0]).max()) for r in res.values()))
    s0 = {name: (*ix.stats(), ix.i8_served()) for name, ix in ixs.items()}
    med = {(name, B): [] for name in ixs for B in BATCHES}
    for _ in range(a.rounds):
        for name, ix in ixs.items():
            for B in BATCHES:
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    ix.search(q[:B], 40)
                    t.append(time.perf_counter() - t0)
                med[(name, B)].append(statistics.median(t))
    by = n * D * 2
    out = {"rows": n, "d": D, "row_bytes": by, "k": 40, "rounds": a.rounds, "reps": a.reps, "identical_ids": bool(same), "id_positions_that_differ": swaps,
           "max_score_difference": dmax, "forms": {}}
    for name, ix in ixs.items():
        s1 = (*ix.stats(), ix.i8_served())
        f = {"env": FORMS[name], "proof_served": s1[0] - s0[name][0], "failed_proofs": s1[1] - s0[name][1],
             "int8_served": s1[2] - s0[name][2], "int8_planes": ix.i8_planes()}
        for B in BATCHES:
            m, y = med[(name, B)], med[("exact32", B)]
            f[f"B{B}"] = {"ms": round(statistics.median(m) * 1e3, 3), "ms_min_max": [round(min(m) * 1e3, 3), round(max(m) * 1e3, 3)],
                          "row_GBps": round(by / statistics.median(m) / 1e9, 1), "qps": round(B / statistics.median(m), 1),
                          "beats_yardstick": bool(statistics.median(y) - statistics.median(m) > max(y) - min(y))}
        out["forms"][name] = f
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
