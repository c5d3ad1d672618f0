#!/usr/bin/env python3
"""knn_d1280_bw.py [--gib 3.9] [--rounds 7] [--reps 9] -- how fast does the 1280-wide flat scan read HBM, next to the 1024-wide one?

Two flat indexes of EQUAL BYTES (2 044 160 x 1024 and 1 635 328 x 1280 fp16 rows at the default size: both below the 2^21 rows at
which the 1024-wide index would switch to its int8 first stage, so both run the exact 32-query scan, knn_scan_kernel NCH = 8 and NCH =
10) over unit rows that torch generates in HBM and the indexes borrow (attach_device_rows).  One process; every round times top-40
searches of B = 1 and B = 32 on one index, then on the other (host clock around a call that returns host arrays, i.e. ends in a device
synchronise); a round's figure is the median of its repetitions, the report the median of the round medians with their spread (min ..
max), as bytes of rows per second, and the ratio 1280 / 1024.  The search time includes the merge and the copy of 40 results."""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from clip_retrieval_amd.knn import Mi355xIndex  # noqa: E402  pylint: disable=wrong-import-position


def unit_rows(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((n, d), dtype=torch.float16, device="cuda")
    for o in range(0, n, 1 << 18):
        r = torch.randn((min(1 << 18, n - o), d), generator=g, device="cuda")
        x[o:o + len(r)] = (r / r.norm(dim=1, keepdim=True)).half()
    torch.cuda.synchronize()
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=3.9)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    units = int(a.gib * 2**30) // (2 * 1024 * 1280)  # rows come in units of 1280 (1024-wide) and 1024 (1280-wide): equal bytes
    cases = {}
    for d in (1024, 1280):
        n = units * (1280 if d == 1024 else 1024)
        x = unit_rows(n, d, d)
        ix = Mi355xIndex(d, coalesce=False)
        ix.attach_device_rows(x.data_ptr(), n)
        q = x[:: n // 32][:32].float().cpu().numpy()
        cases[d] = (ix, x, q, n * d * 2)
        for B in (1, 32):  # warm-up, and the planted rows come back first
            D, I = ix.search(q[:B], 40)
            assert (I[:, 0] == np.arange(B) * (n // 32)).all(), (d, B, I[:, 0])
    med = {(d, B): [] for d in cases for B in (1, 32)}
    for _ in range(a.rounds):
        for d, (ix, _, q, _) in cases.items():
            for B in (1, 32):
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    ix.search(q[:B], 40)
                    t.append(time.perf_counter() - t0)
                med[(d, B)].append(statistics.median(t))
    out = {"rows": {d: c[3] // (2 * d) for d, c in cases.items()}, "bytes": cases[1024][3], "rounds": a.rounds, "reps": a.reps}
    for (d, B), m in med.items():
        by = cases[d][3]
        out[f"d{d}_B{B}"] = {"ms": round(statistics.median(m) * 1e3, 4), "GBps": round(by / statistics.median(m) / 1e9, 1),
                             "GBps_min_max": [round(by / max(m) / 1e9, 1), round(by / min(m) / 1e9, 1)]}
    for B in (1, 32):
        out[f"ratio_1280_over_1024_B{B}"] = round(out[f"d1280_B{B}"]["GBps"] / out[f"d1024_B{B}"]["GBps"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
