#!/usr/bin/env python3
"""Cost of one query call of the device-resident place index (sship_index_bench: normalise + scan + merge) at
(size, dim, queries) = (4 096, 512, 1), (65 536, 512, 1) and (65 536, 512, 64), top_k 50, the reference's gate (min_score 0.75) and no gate
(min_score -inf: every row a candidate, the selection's worst case).  Several rounds, the median of each; milliseconds, and the database
bytes (size * dim * 4) over the time as a fraction of the HBM rate: 8.0 TB/s peak, 6.29 TB/s measured with a float4 copy.  A call with Q
queries reads the database once per tile of 16 queries, so the fraction of a 64-query call can exceed 1 only through the caches.
usage: python scripts/index_query_time.py [--out FILE]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superslam_amd import PlaceIndex, _lib  # noqa: E402

ROUNDS, ITERS, TOP_K = 7, 20, 50
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
SHAPES = ((4096, 512, 1), (65536, 512, 1), (65536, 512, 64))


def measure(size, dim, queries):
    ix = PlaceIndex(dim, size, max_queries=queries, max_top_k=TOP_K)
    assert ix.initialize(), ix.last_error
    g = torch.Generator().manual_seed(0)
    step = 8192
    for lo in range(0, size, step):
        n = min(step, size - lo)
        assert ix.add(range(lo, lo + n), torch.randn((n, dim), generator=g).cuda()), ix.last_error
    q = torch.randn((queries, dim), generator=g).cuda()
    row = {"size": size, "dim": dim, "queries": queries, "top_k": TOP_K, "rounds": ROUNDS, "iters": ITERS}
    for name, min_score in (("gate_0.75", 0.75), ("no_gate", float("-inf"))):
        out = ix.query_batch(q, 0, TOP_K, min_score)
        torch.cuda.synchronize()
        ms = [ix.bench(ITERS) for _ in range(ROUNDS)]
        med = statistics.median(ms)
        rate = size * dim * 4 / (med * 1e-3)
        row[name] = {"ms": round(med, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "db_bytes_per_s": round(rate),
                     "of_hbm_peak": round(rate / HBM_PEAK, 3), "of_hbm_copy": round(rate / HBM_COPY, 3), "mean_count": float(out[2].float().mean())}
    ix.close()
    return row


def main():
    _lib.init()
    out = {"what": "sship_index_bench (k_index_normalize + k_index_scan + k_index_merge); milliseconds per query call, database bytes / time against HBM",
           "runs": [measure(*s) for s in SHAPES]}
    print(json.dumps(out), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
