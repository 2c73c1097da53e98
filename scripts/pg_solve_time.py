#!/usr/bin/env python3
"""Cost of the pose-graph optimiser: 256 graphs of 512 nodes with 16 loops (one per workgroup of the launch), one graph of 4 096 nodes with
0, 16 and 128 loops (the lone chain: its segments are walked node by node by one wave each, and with 128 loops the separator system has
order up to 1 536), and the two gather stages.  The solve is timed by sship_pg_bench (k_pg_solve, one launch), the gather stages by device
events here; 7 rounds (fewer where one launch is so long that 7 would pass 30 s; recorded), the median of each; milliseconds, next to the 512-pair front-end step of the README (90.9 ms), with the trials the
solves took.  Scenes are the tests' generator's: a biased, noisy circuit with true loops, the bias scaled to the chain's length.
usage: python scripts/pg_solve_time.py [--out FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pg_ref as R  # noqa: E402  (the seeded generator of the tests)
from superslam_amd import PoseGraph, _lib  # noqa: E402

ROUNDS = 7
BUDGET_MS = 30e3    # per configuration; a configuration whose launch is long gets fewer rounds (recorded)
STEP_MS = 90.9      # README: the 512-pair front-end step


def timed(fn, iters):
    out = []
    for _ in range(ROUNDS):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def measure(graphs, nodes, loops, iters, gather=False):
    L = max(loops, 1) if gather else loops
    pg = PoseGraph(nodes, L, graphs)
    assert pg.initialize(), pg.last_error
    # 4 scenes, tiled over the batch.  The generator's per-step bias is scaled so that it integrates to 0.08 rad / 0.4 m over the chain
    # whatever its length (at the generator's own 0.002 rad per step a 4 096-node chain winds up by many radians and no solve converges)
    bias = (min(0.002, 0.08 / nodes), min(0.01, 0.4 / nodes))
    scenes = [R.make_graph(7000 + w, nodes, loops=loops, max_loops=L, radius=nodes / 12.0, bias=bias) for w in range(min(graphs, 4))]
    pick = [scenes[w % len(scenes)] for w in range(graphs)]
    t = lambda key, dt: torch.from_numpy(np.stack([np.asarray(getattr(g, key), dt) for g in pick])).cuda()  # noqa: E731
    pose0, oz = t("pose0", np.float64), t("odom_z", np.float64)
    loop = (t("loop_ij", np.int32), t("loop_z", np.float64), t("loop_sigma", np.float64), t("loop_k2", np.float64)) if L else (None,) * 4
    out = pg.optimize_batch(pose0, oz, *loop, loop_enable=t("loop_enable", np.uint8) if L else None)
    torch.cuda.synchronize()
    stats = out.stats.cpu().numpy()
    first = pg.bench(1)                                        # one launch costs up to max_iterations trials: the rounds follow its length
    rounds = ROUNDS if first * 2 * iters * ROUNDS < BUDGET_MS else max(1, int(BUDGET_MS / (first * 2 * iters)))
    print(f"{graphs} x {nodes} nodes, {loops} loops: {first:.1f} ms per launch, {rounds} round(s)", file=sys.stderr, flush=True)
    solve = [pg.bench(iters) for _ in range(rounds)]
    s = statistics.median(solve)
    rec = {"graphs": graphs, "nodes": nodes, "loops": loops, "rounds": rounds, "iters": iters, "solve_ms": round(s, 4),
           "solve_ms_min_max": [round(min(solve), 4), round(max(solve), 4)], "mean_trials": float(stats[:, 2].mean()),
           "statuses": {int(k): int((stats[:, 3] == k).sum()) for k in np.unique(stats[:, 3])},
           "frontend_step_ms": STEP_MS, "solve_share_of_step": round(s / STEP_MS, 4)}
    if gather:
        frm, to = loop[0][:, :, 0].contiguous(), loop[0][:, :, 1].contiguous()
        st = torch.tensor([200, 120, 4, 0], dtype=torch.int32, device="cuda").repeat(graphs, L, 1).contiguous()
        od = timed(lambda: pg.odometry_from_poses(pose0), 20)
        lp = timed(lambda: pg.loops_from_pose_solver(frm, to, loop[1], st), 20)
        rec.update(odometry_stage_ms=round(statistics.median(od), 4), loop_stage_ms=round(statistics.median(lp), 4))
    pg.close()
    return rec


def main():
    _lib.init()
    out = {"what": "k_pg_solve (sship_pg_bench) and the two gather stages (device events), milliseconds per call, the median of each run's "
                   "`rounds` rounds, next to the 512-pair front-end step; a run that ends at ITER_CAP times max_iterations trials, not a "
                   "solve that converges",
           "runs": [measure(256, 512, 16, 2, gather=True), measure(1, 4096, 0, 1), measure(1, 4096, 16, 1), measure(1, 4096, 128, 1)]}
    print(json.dumps(out), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
