#!/usr/bin/env python3
"""Cost of the nearest-neighbour matcher's keypoint-window gate: sship_nn_bench of the gated launches (k_nn_stream_gated + k_nn_final_gated)
against the ungated ones (k_nn_stream + k_nn_final) in one process, on the same descriptors - 64 pairs x 600 keypoints, every set full,
keypoints uniform in a 1376 x 376 image.  One handle per variant (a handle replays its own last call); the variants alternate inside every
round, several rounds, the median of each; one JSON line.  The gated pass issues the same MFMAs plus 32 fp32 window tests per lane per
tile: that is what the ratio is to be read against.
usage: python scripts/nn_gate_time.py [--out FILE]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superslam_amd import NNMatcher, _lib  # noqa: E402

PAIRS, K, ROUNDS, ITERS = 64, 600, 9, 200
INF = float("inf")
GATES = {"ungated": None, "open": (-INF, INF, -INF, INF), "stereo": (1.0, 64.0, -2.0, 2.0), "window": (-24.0, 24.0, -24.0, 24.0)}


def main():
    _lib.init()
    g = torch.Generator().manual_seed(0)
    kp = (torch.rand((2 * PAIRS, K, 3), generator=g) * torch.tensor([1376.0, 376.0, 1.0])).cuda()
    ds = torch.nn.functional.normalize(torch.randn((2 * PAIRS, K, 256), generator=g), dim=-1).half().cuda()
    n = torch.full((2 * PAIRS,), K, dtype=torch.int32).cuda()
    handles, keep, matched = {}, {}, {}
    for name, gate in GATES.items():
        nn = NNMatcher(K, PAIRS, gate=gate)
        assert nn.initialize(), nn.last_error
        keep[name] = nn.match_batch_device(n, ds, kp=kp)        # the call that sship_nn_bench replays; its outputs stay alive
        handles[name] = nn
    torch.cuda.synchronize()
    for name in GATES:
        matched[name] = int((keep[name][0] >= 0).sum())
    assert torch.equal(keep["open"][0], keep["ungated"][0]) and torch.equal(keep["open"][1], keep["ungated"][1])
    for nn in handles.values():
        nn.bench(ITERS)                                         # warm every variant before the timed rounds
    us = {name: [] for name in GATES}
    for _ in range(ROUNDS):
        for name, nn in handles.items():
            us[name].append(nn.bench(ITERS) * 1e3)
    med = {name: statistics.median(v) for name, v in us.items()}
    out = {"what": "sship_nn_bench, gated launches vs ungated launches on the same descriptors; microseconds per call (two launches)",
           "pairs": PAIRS, "max_keypoints": K, "rounds": ROUNDS, "iters": ITERS,
           "us": {name: round(med[name], 1) for name in GATES},
           "us_min_max": {name: [round(min(v), 1), round(max(v), 1)] for name, v in us.items()},
           "gated_over_ungated": {name: round(med[name] / med["ungated"], 3) for name in GATES if name != "ungated"},
           "matched_rows": matched}
    for nn in handles.values():
        nn.close()
    print(json.dumps(out), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
