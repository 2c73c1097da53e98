#!/usr/bin/env python3
"""Cost of the RANSAC pose seed at the throughput path's size: 512 pairs x 2 048 observations x 512 hypotheses, and a lone pair of the same
size (its hypotheses spread over 2 workgroups), with 512 and with 8 192 hypotheses (32 workgroups).  Seeded scenes with motions up to
25 degrees / 4 m, 0.5 px noise and 60 % outliers.  Both launches (k_ransac_score, k_ransac_finish) together: sship_ransac_bench; several
rounds, the median; milliseconds, next to the 512-pair front-end step of the README (90.9 ms) and as a share of it.
usage: python scripts/ransac_time.py [--out FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pose_ref as P  # noqa: E402
import _ransac_ref as R  # noqa: E402  (the seeded generator of the tests)
from superslam_amd import RansacVerifier, _lib  # noqa: E402

ROUNDS, ITERS = 7, 10
STEP_MS = 90.9      # README: the 512-pair front-end step


def measure(pairs, n_obs, hypotheses):
    cam = P.Camera()
    rv = RansacVerifier(cam.tuple(), n_obs, pairs, num_hypotheses=hypotheses)
    assert rv.initialize(), rv.last_error
    scenes = [R.make_pair(9100 + p, n_obs, outliers=0.6) for p in range(min(pairs, 16))]      # 16 scenes, tiled over the batch
    pick = [scenes[p % len(scenes)] for p in range(pairs)]
    t = lambda key: torch.from_numpy(np.stack([d[key] for d in pick])).cuda()
    pts, ms, va = t("points"), t("meas"), t("valid")
    out = rv.solve_batch(pts, ms, va)
    torch.cuda.synchronize()
    stats = out.stats.cpu().numpy()
    times = [rv.bench(ITERS) for _ in range(ROUNDS)]
    rv.close()
    s = statistics.median(times)
    evals = pairs * n_obs * hypotheses
    return {"pairs": pairs, "observations": n_obs, "hypotheses": hypotheses, "rounds": ROUNDS, "iters": ITERS, "solve_ms": round(s, 4),
            "solve_ms_min_max": [round(min(times), 4), round(max(times), 4)], "observation_evaluations_per_ns": round(evals / (s * 1e6), 3),
            "mean_inliers": float(stats[:, 1].mean()), "statuses": {int(k): int((stats[:, 3] == k).sum()) for k in np.unique(stats[:, 3])},
            "frontend_step_ms": STEP_MS, "solve_share_of_step": round(s / STEP_MS, 4)}


def main():
    _lib.init()
    out = {"what": "k_ransac_score + k_ransac_finish (sship_ransac_bench), milliseconds per call, next to the 512-pair front-end step",
           "runs": [measure(512, 2048, 512), measure(1, 2048, 512), measure(1, 2048, 8192)]}
    print(json.dumps(out), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
