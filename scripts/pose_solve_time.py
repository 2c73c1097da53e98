#!/usr/bin/env python3
"""Cost of the pose-only stereo solver at the throughput path's size: 512 pairs with 1 024 and with 2 048 observations each (seeded scenes,
0.5 px noise, 30 % outliers on every second pair, from the identity pose).  The solve (k_pose_solve, one launch: sship_pose_bench) and the
gather (k_pose_gather, one launch, device events here) are timed apart; several rounds, the median of each; milliseconds, next to the
512-pair front-end step of the README (90.9 ms) and as a share of it, and the mean number of trials the solves took.
usage: python scripts/pose_solve_time.py [--out FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pose_ref as P  # noqa: E402  (the seeded generator of the tests)
from superslam_amd import PoseSolver, _lib  # noqa: E402

PAIRS, ROUNDS, ITERS = 512, 7, 10
STEP_MS = 90.9      # README: the 512-pair front-end step of the parent commit


def measure(n_obs):
    cam = P.Camera()
    ps = PoseSolver(cam.tuple(), n_obs, PAIRS)
    assert ps.initialize(), ps.last_error
    scenes = [P.make_pair(9000 + p, n_obs, outliers=0.3 if p % 2 else 0.0) for p in range(16)]      # 16 scenes, tiled over the batch
    pick = [scenes[p % 16] for p in range(PAIRS)]
    t = lambda key: torch.from_numpy(np.stack([d[key] for d in pick])).cuda()
    pts, ms, va = t("points"), t("meas"), t("valid")
    out = ps.solve_batch(pts, ms, va)
    torch.cuda.synchronize()
    stats = out.stats.cpu().numpy()
    solve = [ps.bench(ITERS) for _ in range(ROUNDS)]
    # the gather on the same sizes: every keypoint matched, every point with depth
    stereo = torch.rand((PAIRS, n_obs, 3), device="cuda") * 1000 + 100
    stereo[:, :, 1] = stereo[:, :, 0] - 20
    hd = torch.ones((PAIRS, n_obs), dtype=torch.uint8, device="cuda")
    m0 = torch.arange(n_obs, dtype=torch.int32, device="cuda").repeat(PAIRS, 1).contiguous()
    n = torch.full((PAIRS,), n_obs, dtype=torch.int32, device="cuda")
    gather = []
    for _ in range(ROUNDS):
        ps.obs_from_matches(stereo, hd, stereo, hd, m0, n, n)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            ps.obs_from_matches(stereo, hd, stereo, hd, m0, n, n)
        e1.record()
        e1.synchronize()
        gather.append(e0.elapsed_time(e1) / ITERS)
    ps.close()
    s, g = statistics.median(solve), statistics.median(gather)
    return {"pairs": PAIRS, "observations": n_obs, "rounds": ROUNDS, "iters": ITERS, "solve_ms": round(s, 4),
            "solve_ms_min_max": [round(min(solve), 4), round(max(solve), 4)], "gather_ms": round(g, 4),
            "gather_ms_min_max": [round(min(gather), 4), round(max(gather), 4)], "mean_trials": float(stats[:, 2].mean()),
            "statuses": {int(k): int((stats[:, 3] == k).sum()) for k in np.unique(stats[:, 3])},
            "frontend_step_ms": STEP_MS, "solve_share_of_step": round(s / STEP_MS, 4), "gather_share_of_step": round(g / STEP_MS, 4)}


def main():
    _lib.init()
    out = {"what": "k_pose_solve (sship_pose_bench) and k_pose_gather (device events), milliseconds per call of 512 pairs, next to the 512-pair "
                   "front-end step", "runs": [measure(n) for n in (1024, 2048)]}
    print(json.dumps(out), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
