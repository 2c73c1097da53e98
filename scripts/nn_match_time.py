#!/usr/bin/env python3
"""Cost of the mutual nearest-neighbour matcher (sship_nn_bench) next to what it is measured against, in one run and on the same handle
sizes: the two assignment passes of LightGlue (sship_lg_bench_stage 6 + 7: the same similarity tiles, computed twice) and a full LightGlue
call.  64 pairs and one pair, 600 and 1024 keypoints, every set full; several alternating rounds, the median of each; one JSON line.
usage: python scripts/nn_match_time.py [--out FILE]"""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superslam_amd import LightGlue, NNMatcher, _lib  # noqa: E402
from superslam_amd.weights import make_lightglue_weights, save_safetensors  # noqa: E402

ROUNDS, ITERS = 7, 20
PARAMS = {"nn_mutual": (0.0, 0.0, True), "ratio_distance_mutual": (0.8, 0.7, True)}


def lg_stage(lg, stage):
    ms = C.c_float(0)
    _lib.check(_lib.lib().sship_lg_bench_stage(lg._h, stage, ITERS, C.byref(ms)))
    return ms.value * 1e3


def lg_call(lg, kp, n, ds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        lg.match_batch_device(kp, n, ds)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / ITERS * 1e3


def measure(weights, pairs, k):
    lg = LightGlue(weights, 1376, 376, max_keypoints=k, max_pairs=pairs)
    assert lg.initialize(), lg.last_error
    nn = NNMatcher(k, pairs)
    assert nn.initialize(), nn.last_error
    g = torch.Generator().manual_seed(0)
    kp = (torch.rand((2 * pairs, k, 3), generator=g) * torch.tensor([1376.0, 376.0, 1.0])).cuda()
    ds = torch.nn.functional.normalize(torch.randn((2 * pairs, k, 256), generator=g), dim=-1).half().cuda()
    n = torch.full((2 * pairs,), k, dtype=torch.int32).cuda()
    lg.match_batch_device(kp, n, ds)
    m, s = nn.match_batch_device(n, ds)
    torch.cuda.synchronize()
    us = {name: [] for name in (*PARAMS, "lg_assign_lse", "lg_assign_arg", "lg_call")}
    for _ in range(ROUNDS):
        for name, p in PARAMS.items():
            nn.set_params(*p)
            us[name].append(nn.bench(ITERS) * 1e3)
        us["lg_assign_lse"].append(lg_stage(lg, 6))
        us["lg_assign_arg"].append(lg_stage(lg, 7))
        us["lg_call"].append(lg_call(lg, kp, n, ds))
    med = {name: statistics.median(v) for name, v in us.items()}
    target = med["lg_assign_lse"] + med["lg_assign_arg"]
    row = {"pairs": pairs, "max_keypoints": k, "rounds": ROUNDS, "iters": ITERS,
           "nn_us": {name: round(med[name], 1) for name in PARAMS},
           "nn_us_min_max": {name: [round(min(us[name]), 1), round(max(us[name]), 1)] for name in PARAMS},
           "lg_assign_lse_us": round(med["lg_assign_lse"], 1), "lg_assign_arg_us": round(med["lg_assign_arg"], 1),
           "target_us": round(target, 1), "nn_over_target": round(med["nn_mutual"] / target, 3), "target_met": bool(med["nn_mutual"] <= target),
           "lg_call_us": round(med["lg_call"], 1), "lg_call_over_nn": round(med["lg_call"] / med["nn_mutual"], 1)}
    lg.close(); nn.close()
    return row


def main():
    _lib.init()
    d = tempfile.mkdtemp()
    weights = os.path.join(d, "lg.safetensors")
    save_safetensors(make_lightglue_weights(1), weights)
    out = {"what": "sship_nn_bench (k_nn_stream + k_nn_final) vs sship_lg_bench_stage 6 + 7 and a full sship_lg_match_batch_device call; microseconds",
           "runs": [measure(weights, pairs, k) for pairs in (64, 1) for k in (600, 1024)]}
    print(json.dumps(out), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
