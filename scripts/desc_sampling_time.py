#!/usr/bin/env python3
"""Cost of the bilinear descriptor head (sship_sp_set_descriptor_sampling): sship_sp_bench_layer(14) in both modes, at a throughput batch and
at one stereo pair of 1376x376, 600 keypoints.  Several alternating rounds, the median of each mode; one JSON line.
usage: python scripts/desc_sampling_time.py [--out FILE]"""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superslam_amd import SuperPoint, _lib  # noqa: E402
from superslam_amd.synth import make_stereo_pair  # noqa: E402
from superslam_amd.weights import make_superpoint_weights, save_safetensors  # noqa: E402

H, W, K, ROUNDS, ITERS = 376, 1376, 600, 7, 20


def measure(sp, batch):
    l, r = make_stereo_pair(H, W, 1234)
    imgs = torch.from_numpy(np.stack([l, r] * (batch // 2))).cuda()
    imgs = torch.stack([torch.roll(imgs[i], i * 7, 0) for i in range(batch)])
    sp.extract_batch_device(imgs)
    torch.cuda.synchronize()
    ms = {"nearest": [], "bilinear": []}
    for _ in range(ROUNDS):
        for mode in ("nearest", "bilinear"):
            sp.set_descriptor_sampling(mode)
            t = C.c_float(0)
            _lib.check(_lib.lib().sship_sp_bench_layer(sp._h, 14, batch, H, W, ITERS, C.byref(t), None))
            ms[mode].append(t.value * 1e3)
    sp.set_descriptor_sampling("nearest")
    med = {m: statistics.median(v) for m, v in ms.items()}
    return {"batch": batch, "nearest_us": round(med["nearest"], 1), "bilinear_us": round(med["bilinear"], 1),
            "ratio": round(med["bilinear"] / med["nearest"], 2), "rounds": ROUNDS, "iters": ITERS,
            "nearest_us_min_max": [round(min(ms["nearest"]), 1), round(max(ms["nearest"]), 1)],
            "bilinear_us_min_max": [round(min(ms["bilinear"]), 1), round(max(ms["bilinear"]), 1)]}


def main():
    _lib.init()
    d = tempfile.mkdtemp()
    save_safetensors(make_superpoint_weights(0), os.path.join(d, "sp.safetensors"))
    out = {"shape": [H, W], "max_keypoints": K, "layer": 14, "runs": []}
    for batch in (128, 2):
        sp = SuperPoint(os.path.join(d, "sp.safetensors"), K, 0.005, 4, max_batch=batch)
        assert sp.initialize(), sp.last_error
        out["runs"].append(measure(sp, batch))
        sp.close()
    line = json.dumps(out)
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
