#!/usr/bin/env python3
"""Cost of the window smoother at the throughput path's size: 1 window and 512 windows of 8 keyframes x 600 rows (the generator's scenes:
0.5 px noise, 10 % gross outliers on later views, start poses 0.02 rad / 0.15 m off).  The solve (k_ba_solve, one launch: sship_ba_bench)
and the track builder (k_ba_tracks, one launch, device events here) are timed apart; several rounds, the median of each; milliseconds, next
to the 512-pair front-end step of the README (90.9 ms), and the mean number of trials the solves took.
usage: python scripts/ba_solve_time.py [--out FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _ba_ref as B  # noqa: E402  (the seeded generator of the tests)
import _pose_ref as P  # noqa: E402
from superslam_amd import WindowSmoother, _lib  # noqa: E402

K, N, ROUNDS = 8, 600, 5
STEP_MS = 90.9      # README: the 512-pair front-end step


def measure(windows, iters):
    ws = WindowSmoother(P.Camera().tuple(), K, N, K * N, windows)
    assert ws.initialize(), ws.last_error
    scenes = [B.make_window(9000 + w, K, K, N, K * N, n_tracks=1600, outliers=0.1) for w in range(min(windows, 8))]      # 8 scenes, tiled over the batch
    pick = [scenes[w % len(scenes)] for w in range(windows)]
    t = lambda key, dt: torch.from_numpy(np.stack([np.asarray(d[key], dt) for d in pick])).cuda()
    meas, track, pose0 = t("meas", np.float32), t("track", np.int32), t("pose0", np.float64)
    out = ws.solve_batch(meas, track, pose0)
    torch.cuda.synchronize()
    stats = out.stats.cpu().numpy()
    solve = [ws.bench(iters) for _ in range(ROUNDS)]
    hd = torch.ones((windows, K, N), dtype=torch.uint8, device="cuda")
    m0 = torch.arange(N, dtype=torch.int32, device="cuda").repeat(windows, K - 1, 1).contiguous()
    n = torch.full((windows, K), N, dtype=torch.int32, device="cuda")
    tracks = []
    for _ in range(ROUNDS):
        ws.tracks_from_matches(hd, m0, n)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            ws.tracks_from_matches(hd, m0, n)
        e1.record()
        e1.synchronize()
        tracks.append(e0.elapsed_time(e1) / iters)
    ws.close()
    s, g = statistics.median(solve), statistics.median(tracks)
    return {"windows": windows, "keyframes": K, "rows": N, "rounds": ROUNDS, "iters": iters, "solve_ms": round(s, 4),
            "solve_ms_min_max": [round(min(solve), 4), round(max(solve), 4)], "tracks_ms": round(g, 4),
            "tracks_ms_min_max": [round(min(tracks), 4), round(max(tracks), 4)], "mean_observations": float(stats[:, 0].mean()),
            "mean_landmarks": float(stats[:, 1].mean()), "mean_trials": float(stats[:, 2].mean()),
            "statuses": {int(k): int((stats[:, 3] == k).sum()) for k in np.unique(stats[:, 3])},
            "frontend_step_ms": STEP_MS, "solve_share_of_step": round(s / STEP_MS, 4)}


def main():
    _lib.init()
    out = {"what": "k_ba_solve (sship_ba_bench) and k_ba_tracks (device events), milliseconds per call of 1 and of 512 windows of 8 keyframes x "
                   "600 rows, next to the 512-pair front-end step", "runs": [measure(1, 5), measure(512, 2)]}
    print(json.dumps(out), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
